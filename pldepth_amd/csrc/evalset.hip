// Test-set evaluation on the GPU: what the reference's evaluation side does image by image and
// point by point in Python, as one launch per call for the whole set of images:
//   generate_ordinal_pairs   pldepth/data/providers/generic_ranking_provider.py:91-109
//   generate_rankings        :190-212
//   the ordinal pair error over the stored table (the reason :108 keeps z0 and z1)
//   skimage.transform.resize as the Ibims / DIODE / TUM loaders call it
//                            pldepth/data/dao/ibims.py:20-21, diode.py:34, tum.py:33-35
// The random coordinates come from the host (the reference's global numpy RNG, in its order).
// Pairs and rankings only gather, compare and order, so they equal the NumPy restatement
// (tests/evalset_ref.py) bit for bit; the resize accumulates in double and rounds once.
#include <climits>
#include <cmath>

#include "common.h"

namespace pld {

constexpr int EV_T = 256;
constexpr long EV_MAX_PIXELS = 1L << 24;  // flat indices are stored as float32

struct RelThresholds {
  float hi, lo;
  int plain;  // threshold=None: d1 > d2, d1 < d2
};

static RelThresholds rel_thresholds(double tau) {
  RelThresholds t;
  t.plain = tau < 0.0;
  t.hi = (float)(1.0 + tau);
  t.lo = (float)(1.0 / (1.0 + tau));
  return t;
}

__device__ __forceinline__ int relation(float z0, float z1, RelThresholds t, int invert) {
  const int r = t.plain ? (z0 > z1) - (z0 < z1) : depth_relation32(z0, z1, t.hi, t.lo);
  return invert ? -r : r;
}

// ---------------------------------------------------------------------------------------------
// ordinal pairs: one thread per pair
// ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(EV_T) void ordinal_pairs_kernel(const float* __restrict__ gt, int h,
                                                             int w, const int4* __restrict__ xy,
                                                             int P, long total, RelThresholds t,
                                                             int invert, float* __restrict__ out) {
  const long id = (long)blockIdx.x * EV_T + threadIdx.x;
  if (id >= total) return;
  const float* g = gt + (id / P) * h * w;
  const int4 c = xy[id];
  const bool in0 = c.x >= 0 && c.x < h && c.y >= 0 && c.y < w;
  const bool in1 = c.z >= 0 && c.z < h && c.w >= 0 && c.w < w;
  const float z0 = in0 ? g[(long)c.x * w + c.y] : 0.f;
  const float z1 = in1 ? g[(long)c.z * w + c.w] : 0.f;
  float* o = out + id * 5;
  o[0] = (float)(c.x * w + c.y);
  o[1] = (float)(c.z * w + c.w);
  o[2] = (float)relation(z0, z1, t, invert);
  o[3] = z0;
  o[4] = z1;
}

// ---------------------------------------------------------------------------------------------
// rankings: one 64-lane wave per list, one entry per lane. The position of an entry in the
// stable ascending order is the number of entries that sort before it: smaller depth, or the
// same depth at an earlier list position (NaN after every number). Descending is that order
// reversed.
// ---------------------------------------------------------------------------------------------
__device__ __forceinline__ bool sorts_before(float a, int ia, float b, int ib) {
  const bool an = a != a, bn = b != b;
  if (an || bn) return an == bn ? ia < ib : bn;
  return a < b || (a == b && ia < ib);
}

__global__ __launch_bounds__(EV_T) void depth_rankings_kernel(const float* __restrict__ gt,
                                                              long hw, const int* __restrict__ idx,
                                                              int R, int L, long lists, int invert,
                                                              float* __restrict__ out) {
  const int lane = threadIdx.x & 63;
  const long list = (long)blockIdx.x * (EV_T / 64) + (threadIdx.x >> 6);
  if (list >= lists) return;  // the whole wave leaves
  const float* g = gt + (list / R) * hw;
  int p = 0;
  float z = 0.f;
  if (lane < L) {
    p = idx[list * L + lane];
    z = (p >= 0 && p < hw) ? g[p] : 0.f;
  }
  int rank = 0;
  for (int j = 0; j < L; ++j) {
    const float zj = __shfl(z, j, 64);
    rank += sorts_before(zj, j, z, lane) ? 1 : 0;
  }
  if (lane >= L) return;
  const int pos = invert ? rank : L - 1 - rank;
  const float d = invert ? (float)(1.0 / ((double)z + 1.0)) : z;
  float2* o = reinterpret_cast<float2*>(out) + list * L + pos;
  *o = make_float2((float)p, d);
}

// ---------------------------------------------------------------------------------------------
// ordinal pair error: one workgroup per image
// ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(EV_T) void pair_error_kernel(const float* __restrict__ pred, long hw,
                                                          const float* __restrict__ pairs, int P,
                                                          RelThresholds t, int use_tau, int invert,
                                                          int* __restrict__ wrong,
                                                          int* __restrict__ counted) {
  __shared__ int part[2][EV_T / 64];
  const float* p = pred + (long)blockIdx.x * hw;
  const float* tab = pairs + (long)blockIdx.x * P * 5;
  int nw = 0, nc = 0;
  for (int i = threadIdx.x; i < P; i += EV_T) {
    const float* row = tab + (long)i * 5;
    const int rel = use_tau ? relation(row[3], row[4], t, invert)
                            : (row[2] > 0.f) - (row[2] < 0.f);
    if (rel == 0) continue;
    ++nc;
    const float f0 = row[0], f1 = row[1];
    // the comparison on the float is false for NaN; the cast is then not evaluated
    const bool ok = f0 >= 0.f && f0 < (float)hw && f1 >= 0.f && f1 < (float)hw;
    int s = 0;
    if (ok) {
      const float a = p[(long)f0], b = p[(long)f1];
      s = (a > b) - (a < b);
    }
    nw += s != rel;
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    nw += __shfl_xor(nw, o, 64);
    nc += __shfl_xor(nc, o, 64);
  }
  if ((threadIdx.x & 63) == 0) {
    part[0][threadIdx.x >> 6] = nw;
    part[1][threadIdx.x >> 6] = nc;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    int sw = 0, sc = 0;
    for (int k = 0; k < EV_T / 64; ++k) {
      sw += part[0][k];
      sc += part[1][k];
    }
    wrong[blockIdx.x] = sw;
    counted[blockIdx.x] = sc;
  }
}

// ---------------------------------------------------------------------------------------------
// anti-aliased resize: one thread per output element. The linear interpolation reads the blurred
// map at two rows and two columns; each of those is the Gaussian correlation around it.
// ---------------------------------------------------------------------------------------------
// scipy.ndimage 'mirror': d c b | a b c d | c b a
__device__ __forceinline__ int mirror_index(int i, int n) {
  if (n == 1) return 0;
  while (i < 0 || i >= n) i = i < 0 ? -i : 2 * n - 2 - i;
  return i;
}

// the source coordinate of output index o (grid_mode zoom), mirrored into [0, n - 1], as the
// lower neighbour and the weight of the upper one
__device__ __forceinline__ void source_coord(int o, int n_in, int n_out, int& i0, double& f) {
  double s = ((double)o + 0.5) * ((double)n_in / (double)n_out) - 0.5;
  const double top = (double)(n_in - 1);
  if (n_in == 1) s = 0.0;
  while (s < 0.0 || s > top) s = s < 0.0 ? -s : 2.0 * top - s;
  const double fl = floor(s);
  i0 = (int)fl;
  f = s - fl;
}

__global__ __launch_bounds__(EV_T) void resize_antialias_kernel(
    const float* __restrict__ x, int h, int w, int c, int oh, int ow, const double* __restrict__ wy,
    int ry, const double* __restrict__ wx, int rx, long total, float* __restrict__ y) {
  const long id = (long)blockIdx.x * EV_T + threadIdx.x;
  if (id >= total) return;
  const int ch = (int)(id % c);
  long r = id / c;
  const int ox = (int)(r % ow);
  r /= ow;
  const int oy = (int)(r % oh);
  const float* img = x + (r / oh) * h * w * c;
  int y0, x0;
  double fy, fx;
  source_coord(oy, h, oh, y0, fy);
  source_coord(ox, w, ow, x0, fx);
  double acc = 0.0;
  for (int a = 0; a < 2; ++a) {
    const double wa = a ? fy : 1.0 - fy;
    if (wa == 0.0) continue;
    const int ya = mirror_index(y0 + a, h);
    for (int dy = -ry; dy <= ry; ++dy) {
      const float* row = img + (long)mirror_index(ya + dy, h) * w * c + ch;
      double racc = 0.0;
      for (int b = 0; b < 2; ++b) {
        const double wb = b ? fx : 1.0 - fx;
        if (wb == 0.0) continue;
        const int xb = mirror_index(x0 + b, w);
        double bacc = 0.0;
        for (int dx = -rx; dx <= rx; ++dx)
          bacc += wx[dx < 0 ? -dx : dx] * (double)row[(long)mirror_index(xb + dx, w) * c];
        racc += wb * bacc;
      }
      acc += wa * wy[dy < 0 ? -dy : dy] * racc;
    }
  }
  y[id] = (float)acc;
}

}  // namespace pld

using namespace pld;

extern "C" int pld_ordinal_pairs(const float* gt, int n, int h, int w, const int32_t* coords,
                                 int P, double tau, int invert, float* out, void* stream) {
  PLD_CHECK_ARG(gt && coords && out, "pld_ordinal_pairs: null pointer");
  PLD_CHECK_ARG(n > 0 && h > 0 && w > 0 && P > 0, "pld_ordinal_pairs: bad sizes");
  PLD_CHECK_ARG((long)h * w <= EV_MAX_PIXELS,
                "pld_ordinal_pairs: %d x %d pixels, indices are exact in float32 up to 2^24", h, w);
  PLD_CHECK_ARG(tau == tau, "pld_ordinal_pairs: tau is NaN");
  PLD_CHECK_ARG(aligned16(coords), "pld_ordinal_pairs: coords must be 16-byte aligned");
  const long total = (long)n * P;
  PLD_CHECK_ARG(total <= INT_MAX / 5, "pld_ordinal_pairs: too many pairs");
  ordinal_pairs_kernel<<<cdiv(total, EV_T), EV_T, 0, as_stream(stream)>>>(
      gt, h, w, reinterpret_cast<const int4*>(coords), P, total, rel_thresholds(tau), invert, out);
  return check_launch("ordinal_pairs_kernel");
}

extern "C" int pld_depth_rankings(const float* gt, int n, int64_t hw, const int32_t* idx, int R,
                                  int L, int invert, float* out, void* stream) {
  PLD_CHECK_ARG(gt && idx && out, "pld_depth_rankings: null pointer");
  PLD_CHECK_ARG(n > 0 && hw > 0 && R > 0 && L > 0, "pld_depth_rankings: bad sizes");
  PLD_CHECK_ARG(hw <= EV_MAX_PIXELS,
                "pld_depth_rankings: %ld pixels, indices are exact in float32 up to 2^24",
                (long)hw);
  if (L > PLD_RANKING_MAX_L) {
    set_error("pld_depth_rankings: ranking size %d above the limit of %d", L, PLD_RANKING_MAX_L);
    return PLD_ERR_UNSUPPORTED;
  }
  const long lists = (long)n * R;
  PLD_CHECK_ARG(lists <= INT_MAX / (2 * PLD_RANKING_MAX_L), "pld_depth_rankings: too many lists");
  PLD_CHECK_ARG(((uintptr_t)out & 7) == 0, "pld_depth_rankings: out must be 8-byte aligned");
  depth_rankings_kernel<<<cdiv(lists, EV_T / 64), EV_T, 0, as_stream(stream)>>>(
      gt, (long)hw, idx, R, L, lists, invert, out);
  return check_launch("depth_rankings_kernel");
}

extern "C" int pld_ordinal_pair_error(const float* pred, int n, int64_t hw, const float* pairs,
                                      int P, double tau, int use_tau, int invert, int32_t* wrong,
                                      int32_t* counted, void* stream) {
  PLD_CHECK_ARG(pred && pairs && wrong && counted, "pld_ordinal_pair_error: null pointer");
  PLD_CHECK_ARG(n > 0 && hw > 0 && P > 0, "pld_ordinal_pair_error: bad sizes");
  PLD_CHECK_ARG(hw <= EV_MAX_PIXELS,
                "pld_ordinal_pair_error: %ld pixels, indices are exact in float32 up to 2^24",
                (long)hw);
  PLD_CHECK_ARG(!use_tau || tau == tau, "pld_ordinal_pair_error: tau is NaN");
  pair_error_kernel<<<n, EV_T, 0, as_stream(stream)>>>(pred, (long)hw, pairs, P,
                                                      rel_thresholds(use_tau ? tau : 0.0),
                                                      use_tau, invert, wrong, counted);
  return check_launch("pair_error_kernel");
}

extern "C" int pld_resize_antialias(const float* x, int n, int h, int w, int c, int oh, int ow,
                                    const double* wy, int ry, const double* wx, int rx, float* y,
                                    void* stream) {
  PLD_CHECK_ARG(x && wy && wx && y, "pld_resize_antialias: null pointer");
  PLD_CHECK_ARG(n > 0 && h > 0 && w > 0 && c > 0 && oh > 0 && ow > 0 && ry >= 0 && rx >= 0,
                "pld_resize_antialias: bad sizes");
  PLD_CHECK_ARG((long)n * h * w * c < (1L << 31) && (long)n * oh * ow * c < (1L << 31),
                "pld_resize_antialias: tensor too large");
  const long total = (long)n * oh * ow * c;
  resize_antialias_kernel<<<cdiv(total, EV_T), EV_T, 0, as_stream(stream)>>>(
      x, h, w, c, oh, ow, wy, ry, wx, rx, total, y);
  return check_launch("resize_antialias_kernel");
}
