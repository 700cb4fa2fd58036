// Depth-edge metrics of the evaluation pass (the second half), batched over
// images on the GPU:
//   depth_edge_metric   pldepth/active_learning/metrics.py:123-144 (used by calc_depth_metrics
//                       :147-156)
//   auto_canny          pldepth/active_learning/preprocess_utils.py:4-13
// The reference calls OpenCV for the three image operators; they are restated here:
//   cv2.normalize(x, None, 0, 255, NORM_MINMAX).astype(uint8)   minmax_*_kernel
//   cv2.Canny(img, lower, upper) (aperture 3, L1 gradient)       canny_nms_kernel + hysteresis_kernel
//   cv2.distanceTransform(E, DIST_L2, 3)                         chamfer_fixed (per pixel)
// Everything after the 8-bit conversion is integer arithmetic, so every result is independent of
// thread order and equals the CPU restatement (tests/edge_ref.py) bit for bit.
#include <algorithm>
#include <cfloat>
#include <climits>

#include "common.h"

namespace pld {

// ---------------------------------------------------------------------------------------------
// min-max to 8 bit: scale = 255 / (max - min) in double (0 when max - min <= DBL_EPSILON),
// shift = -min * scale, f = (float)((double)x * scale + shift), truncated and clamped to [0, 255]
// (the formula of calc_d's normalisation, metrics.hip, with 255 as the upper bound).
// Two launches of (blocks, n): per-block partial min / max, then every block reduces its image's
// partials and converts its own chunk.
// ---------------------------------------------------------------------------------------------
constexpr int MM_T = 256;
constexpr int MM_MAXB = 64;  // partials per image (workspace: n * MM_MAXB * 2 floats)

__device__ __forceinline__ void block_minmax(float& mn, float& mx, float* rmin, float* rmax) {
  rmin[threadIdx.x] = mn;
  rmax[threadIdx.x] = mx;
  __syncthreads();
  for (int o = MM_T / 2; o > 0; o >>= 1) {
    if ((int)threadIdx.x < o) {
      rmin[threadIdx.x] = fminf(rmin[threadIdx.x], rmin[threadIdx.x + o]);
      rmax[threadIdx.x] = fmaxf(rmax[threadIdx.x], rmax[threadIdx.x + o]);
    }
    __syncthreads();
  }
  mn = rmin[0];
  mx = rmax[0];
}

__global__ __launch_bounds__(MM_T) void minmax_partial_kernel(const float* __restrict__ x, long hw,
                                                              long per, float* __restrict__ part) {
  __shared__ float rmin[MM_T], rmax[MM_T];
  const float* p = x + (long)blockIdx.y * hw;
  const long i0 = (long)blockIdx.x * per;
  const long i1 = i0 + per < hw ? i0 + per : hw;
  float mn = FLT_MAX, mx = -FLT_MAX;
  for (long i = i0 + threadIdx.x; i < i1; i += MM_T) {
    const float v = p[i];
    mn = fminf(mn, v);
    mx = fmaxf(mx, v);
  }
  block_minmax(mn, mx, rmin, rmax);
  if (threadIdx.x == 0) {
    float* o = part + ((long)blockIdx.y * gridDim.x + blockIdx.x) * 2;
    o[0] = mn;
    o[1] = mx;
  }
}

// the product and the sum round separately, as NumPy's two array operations do
__device__ __forceinline__ float scale_shift(float v, double scale, double shift) {
#pragma clang fp contract(off)
  const double t = (double)v * scale;
  return (float)(t + shift);
}

__global__ __launch_bounds__(MM_T) void minmax_map_kernel(const float* __restrict__ x, long hw,
                                                          long per, const float* __restrict__ part,
                                                          uint8_t* __restrict__ out) {
  __shared__ float rmin[MM_T], rmax[MM_T];
  const float* pp = part + (long)blockIdx.y * gridDim.x * 2;
  float mn = FLT_MAX, mx = -FLT_MAX;
  if (threadIdx.x < gridDim.x) {
    mn = pp[2 * threadIdx.x];
    mx = pp[2 * threadIdx.x + 1];
  }
  block_minmax(mn, mx, rmin, rmax);
  const double smin = mn, smax = mx;
  const double scale = (smax - smin) > DBL_EPSILON ? 255.0 / (smax - smin) : 0.0;
  const double shift = -smin * scale;
  const float* p = x + (long)blockIdx.y * hw;
  uint8_t* o = out + (long)blockIdx.y * hw;
  const long i0 = (long)blockIdx.x * per;
  const long i1 = i0 + per < hw ? i0 + per : hw;
  for (long i = i0 + threadIdx.x; i < i1; i += MM_T) {
    const float f = scale_shift(p[i], scale, shift);
    o[i] = (uint8_t)(f > 0.f ? (f < 255.f ? (int)f : 255) : 0);  // NaN -> 0
  }
}

// ---------------------------------------------------------------------------------------------
// auto_canny's thresholds: 256-bin histogram per image (integer atomics: order-independent),
// np.median from its running sum, then lower = int(max(0, lo_factor * v)),
// upper = int(min(255, hi_factor * v)) in double.
// ---------------------------------------------------------------------------------------------
constexpr int HIST_T = 256;
constexpr int HIST_MAXB = 64;

// the histogram's clear is a kernel, not a memset node: the library records none
__global__ __launch_bounds__(HIST_T) void hist_clear_kernel(unsigned* __restrict__ hist, long n) {
  const long i = (long)blockIdx.x * HIST_T + threadIdx.x;
  if (i < n) hist[i] = 0;
}

__global__ __launch_bounds__(HIST_T) void hist_kernel(const uint8_t* __restrict__ img, long hw,
                                                      long per, unsigned* __restrict__ hist) {
  __shared__ unsigned hs[256];
  hs[threadIdx.x] = 0;
  __syncthreads();
  const uint8_t* p = img + (long)blockIdx.y * hw;
  const long i0 = (long)blockIdx.x * per;
  const long i1 = i0 + per < hw ? i0 + per : hw;
  for (long i = i0 + threadIdx.x; i < i1; i += HIST_T) atomicAdd(&hs[p[i]], 1u);
  __syncthreads();
  if (hs[threadIdx.x]) atomicAdd(&hist[(long)blockIdx.y * 256 + threadIdx.x], hs[threadIdx.x]);
}

// one thread per image: the two middle order statistics (the same one when hw is odd)
__global__ __launch_bounds__(64) void median_thresholds_kernel(const unsigned* __restrict__ hist,
                                                               int n, long hw, double lo_factor,
                                                               double hi_factor,
                                                               int* __restrict__ thr) {
  const int img = blockIdx.x * 64 + threadIdx.x;
  if (img >= n) return;
  const unsigned* hg = hist + (long)img * 256;
  const long r1 = (hw - 1) / 2, r2 = hw / 2;
  long cum = 0;
  int a = -1, b = -1;
  for (int v = 0; v < 256; ++v) {
    cum += hg[v];
    if (a < 0 && cum > r1) a = v;
    if (b < 0 && cum > r2) b = v;
  }
  const double med = (double)(a + b) * 0.5;
  const double lo = fmax(0.0, lo_factor * med);
  const double hi = fmin(255.0, hi_factor * med);
  thr[2 * img] = (int)lo;
  thr[2 * img + 1] = (int)hi;
}

// ---------------------------------------------------------------------------------------------
// Canny, gradient and non-maximum suppression. One block per 64 x 16 tile: the u8 tile with a
// replicated 2-pixel border goes to LDS, then |dx| + |dy| of the 3x3 Sobel for the tile plus a
// 1-pixel ring (0 outside the image), then each wave labels whole 64-pixel row segments and
// writes them as two words of the image's strong / weak bit maps (bit i of word k = pixel
// 32 k + i of the row; words per row = 2 * ceil(w / 64), bits beyond w are 0).
// ---------------------------------------------------------------------------------------------
constexpr int NMS_TW = 64, NMS_TH = 16, NMS_T = 256;
constexpr int TG22 = 13573;  // tan(22.5 deg) * 2^15

__global__ __launch_bounds__(NMS_T) void canny_nms_kernel(const uint8_t* __restrict__ img, int h,
                                                          int w, const int* __restrict__ thr,
                                                          int lo_arg, int hi_arg,
                                                          unsigned* __restrict__ strong,
                                                          unsigned* __restrict__ weak) {
  __shared__ uint8_t px[NMS_TH + 4][NMS_TW + 4];
  __shared__ int mag[NMS_TH + 2][NMS_TW + 2];
  const int im = blockIdx.z;
  const uint8_t* p = img + (long)im * h * w;
  const int x0 = blockIdx.x * NMS_TW, y0 = blockIdx.y * NMS_TH;
  int lo = thr ? thr[2 * im] : lo_arg, hi = thr ? thr[2 * im + 1] : hi_arg;
  if (lo > hi) {  // cv2.Canny swaps them
    const int t = lo;
    lo = hi;
    hi = t;
  }
  for (int i = threadIdx.x; i < (NMS_TH + 4) * (NMS_TW + 4); i += NMS_T) {
    const int ly = i / (NMS_TW + 4), lx = i % (NMS_TW + 4);
    const int y = min(max(y0 + ly - 2, 0), h - 1), x = min(max(x0 + lx - 2, 0), w - 1);
    px[ly][lx] = p[(long)y * w + x];
  }
  __syncthreads();
  // px[ly + 2][lx + 2] is pixel (y0 + ly, x0 + lx); mag[ly + 1][lx + 1] its gradient magnitude
  for (int i = threadIdx.x; i < (NMS_TH + 2) * (NMS_TW + 2); i += NMS_T) {
    const int ly = i / (NMS_TW + 2) - 1, lx = i % (NMS_TW + 2) - 1;
    const int y = y0 + ly, x = x0 + lx;
    int m = 0;
    if (y >= 0 && y < h && x >= 0 && x < w) {
      const uint8_t(*q)[NMS_TW + 4] = px;
      const int cy = ly + 2, cx = lx + 2;
      const int dx = (q[cy - 1][cx + 1] + 2 * q[cy][cx + 1] + q[cy + 1][cx + 1]) -
                     (q[cy - 1][cx - 1] + 2 * q[cy][cx - 1] + q[cy + 1][cx - 1]);
      const int dy = (q[cy + 1][cx - 1] + 2 * q[cy + 1][cx] + q[cy + 1][cx + 1]) -
                     (q[cy - 1][cx - 1] + 2 * q[cy - 1][cx] + q[cy - 1][cx + 1]);
      m = abs(dx) + abs(dy);
    }
    mag[ly + 1][lx + 1] = m;
  }
  __syncthreads();
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int wpr = 2 * gridDim.x;
  for (int ly = wave; ly < NMS_TH; ly += NMS_T / 64) {
    const int y = y0 + ly, x = x0 + lane;
    if (y >= h) break;  // the same for the whole wave
    bool cand = false, is_strong = false;
    if (x < w) {
      const int cy = ly + 2, cx = lane + 2;
      const int dx = (px[cy - 1][cx + 1] + 2 * px[cy][cx + 1] + px[cy + 1][cx + 1]) -
                     (px[cy - 1][cx - 1] + 2 * px[cy][cx - 1] + px[cy + 1][cx - 1]);
      const int dy = (px[cy + 1][cx - 1] + 2 * px[cy + 1][cx] + px[cy + 1][cx + 1]) -
                     (px[cy - 1][cx - 1] + 2 * px[cy - 1][cx] + px[cy - 1][cx + 1]);
      const int my = ly + 1, mx = lane + 1;
      const int m = mag[my][mx];
      if (m > lo) {
        const int ax = abs(dx), ay = abs(dy) << 15;
        const int t22 = ax * TG22;
        if (ay < t22) {
          cand = m > mag[my][mx - 1] && m >= mag[my][mx + 1];
        } else if (ay > t22 + (ax << 16)) {
          cand = m > mag[my - 1][mx] && m >= mag[my + 1][mx];
        } else {
          const int s = ((dx ^ dy) < 0) ? -1 : 1;
          cand = m > mag[my - 1][mx - s] && m > mag[my + 1][mx + s];
        }
        is_strong = cand && m > hi;
      }
    }
    const unsigned long long bs = __ballot(is_strong);
    const unsigned long long bw = __ballot(cand && !is_strong);
    if (lane == 0) {
      const long o = ((long)im * h + y) * wpr + 2 * blockIdx.x;
      strong[o] = (unsigned)bs;
      strong[o + 1] = (unsigned)(bs >> 32);
      weak[o] = (unsigned)bw;
      weak[o + 1] = (unsigned)(bw >> 32);
    }
  }
}

// ---------------------------------------------------------------------------------------------
// Canny, hysteresis: the closure of the strong set over 8-connected weak pixels. A fixpoint, so
// the result does not depend on the order of evaluation. One workgroup per image holds both bit
// maps in LDS (2 x 32 KiB at 512 x 512, which sets PLD_EDGE_MAX_DIM). Every thread owns one word
// column of a band of rows, sweeps it down and then up, and promotes the weak pixels of a word
// that touch a strong pixel in the 3 x 3 words around it, spreading along the row inside the
// word. Only the owner writes a word; a neighbour's word may be read before or after its owner
// updates it in the same sweep, which only moves a promotion to the next sweep: a sweep in which
// no thread changed anything has read final values everywhere. At most h * w sweeps are run.
// ---------------------------------------------------------------------------------------------
constexpr int HYST_T = 1024;
constexpr int HYST_MAX_WORDS = PLD_EDGE_MAX_DIM * (PLD_EDGE_MAX_DIM / 32);

// pixels of `pro` connected to a pixel of `gen` through pixels of `pro` along the word
// (Kogge-Stone fill towards the higher bits and towards the lower bits)
__device__ __forceinline__ unsigned fill_row(unsigned gen, unsigned pro) {
  unsigned g = gen, p = pro;
  g |= p & (g << 1);
  p &= p << 1;
  g |= p & (g << 2);
  p &= p << 2;
  g |= p & (g << 4);
  p &= p << 4;
  g |= p & (g << 8);
  p &= p << 8;
  g |= p & (g << 16);
  unsigned r = gen;
  p = pro;
  r |= p & (r >> 1);
  p &= p >> 1;
  r |= p & (r >> 2);
  p &= p >> 2;
  r |= p & (r >> 4);
  p &= p >> 4;
  r |= p & (r >> 8);
  p &= p >> 8;
  r |= p & (r >> 16);
  return g | r;
}

__device__ __forceinline__ unsigned column3(const unsigned* S, int i, int r, int h, int wpr) {
  unsigned m = S[i];
  if (r > 0) m |= S[i - wpr];
  if (r < h - 1) m |= S[i + wpr];
  return m;
}

__device__ __forceinline__ int relax_word(unsigned* S, unsigned* Wk, int r, int c, int h,
                                          int wpr) {
  const int i = r * wpr + c;
  const unsigned wk = Wk[i];
  if (!wk) return 0;
  const unsigned mc = column3(S, i, r, h, wpr);
  const unsigned ml = c > 0 ? column3(S, i - 1, r, h, wpr) : 0u;
  const unsigned mr = c < wpr - 1 ? column3(S, i + 1, r, h, wpr) : 0u;
  const unsigned seed = wk & (mc | (mc << 1) | (mc >> 1) | (ml >> 31) | (mr << 31));
  if (!seed) return 0;
  const unsigned f = fill_row(seed, wk);
  S[i] |= f;
  Wk[i] = wk & ~f;
  return 1;
}

__global__ __launch_bounds__(HYST_T) void hysteresis_kernel(const unsigned* __restrict__ strong,
                                                            const unsigned* __restrict__ weak,
                                                            int h, int w, int wpr,
                                                            uint8_t* __restrict__ edges,
                                                            int* __restrict__ sweeps_out) {
  __shared__ unsigned S[HYST_MAX_WORDS], Wk[HYST_MAX_WORDS];
  const int im = blockIdx.x, nwords = h * wpr;
  for (int i = threadIdx.x; i < nwords; i += HYST_T) {
    S[i] = strong[(long)im * nwords + i];
    Wk[i] = weak[(long)im * nwords + i];
  }
  __syncthreads();
  const int nband = HYST_T / wpr;
  const int rows = (h + nband - 1) / nband;
  const int c = threadIdx.x % wpr, band = threadIdx.x / wpr;
  const int r0 = band * rows, r1 = min(h, r0 + rows);  // empty for threads beyond the last band
  const long max_sweeps = (long)h * w;
  int sweeps = 0;
  for (long it = 0; it < max_sweeps; ++it) {
    int changed = 0;
    for (int r = r0; r < r1; ++r) changed |= relax_word(S, Wk, r, c, h, wpr);
    for (int r = r1 - 2; r >= r0; --r) changed |= relax_word(S, Wk, r, c, h, wpr);
    ++sweeps;
    if (!__syncthreads_or(changed)) break;
  }
  if (sweeps_out && threadIdx.x == 0) sweeps_out[im] = sweeps;
  uint8_t* e = edges + (long)im * h * w;
  for (int i = threadIdx.x; i < h * w; i += HYST_T) {
    const int y = i / w, x = i % w;
    e[i] = ((S[y * wpr + (x >> 5)] >> (x & 31)) & 1u) ? 255 : 0;
  }
}

// ---------------------------------------------------------------------------------------------
// 3x3 chamfer distance (cv2.distanceTransform DIST_L2, mask 3: 16.16 fixed point, 62587 per
// edge step, 89738 per diagonal step) from a non-zero pixel to the nearest zero pixel inside the
// image, evaluated per pixel: to a zero pixel at offset (dx, dy) it is
// min(|dx|, |dy|) * 89738 + (max - min) * 62587. Rings of growing Chebyshev radius r are
// searched; every pixel of ring r is at least r * 62587 away, which ends the search early.
// INT_MAX when no zero pixel lies within `radius`.
// ---------------------------------------------------------------------------------------------
constexpr int HV_DIST = 62587, DIAG_DIST = 89738;
constexpr int DT_MAX_RADIUS = 10;

__device__ __forceinline__ void chamfer_probe(const uint8_t* __restrict__ m, int h, int w, int y,
                                              int x, int ady, int adx, int& best) {
  if (y < 0 || y >= h || x < 0 || x >= w || m[(long)y * w + x]) return;
  const int lo = min(adx, ady), hi = max(adx, ady);
  best = min(best, lo * DIAG_DIST + (hi - lo) * HV_DIST);
}

__device__ int chamfer_fixed(const uint8_t* __restrict__ m, int h, int w, int y, int x,
                             int radius) {
  int best = INT_MAX;
  for (int r = 1; r <= radius; ++r) {
    if (best <= r * HV_DIST) break;
    for (int t = -r; t <= r; ++t) {
      const int at = abs(t);
      chamfer_probe(m, h, w, y - r, x + t, r, at, best);
      chamfer_probe(m, h, w, y + r, x + t, r, at, best);
      if (at < r) {
        chamfer_probe(m, h, w, y + t, x - r, at, r, best);
        chamfer_probe(m, h, w, y + t, x + r, at, r, best);
      }
    }
  }
  return best;
}

__global__ __launch_bounds__(256) void chamfer_dt3_kernel(const uint8_t* __restrict__ mask, int h,
                                                          int w, int radius, float max_dist,
                                                          float* __restrict__ out) {
  const long hw = (long)h * w;
  const uint8_t* m = mask + (long)blockIdx.y * hw;
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= hw) return;
  float d = 0.f;
  if (m[i]) {
    const int f = chamfer_fixed(m, h, w, (int)(i / w), (int)(i % w), radius);
    if (f != INT_MAX) {
      d = (float)f * (1.0f / 65536.0f);
      if (d > max_dist) d = 0.f;
    }
  }
  out[(long)blockIdx.y * hw + i] = d;
}

// ---------------------------------------------------------------------------------------------
// depth_edge_metric's sums (metrics.py:129-142) without the distance maps: the transform of an
// edge map is non-zero only on its own edges, so e_gt * E_op is non-zero only where both maps
// have an edge. 64-bit integer sums of the fixed-point distances (those above 10 dropped) and
// of the edge counts; one workgroup per image.
// ---------------------------------------------------------------------------------------------
constexpr int EM_T = 1024;
constexpr int DT_CUT = 10 * 65536;  // (float)f / 65536 > 10  <=>  f > 655360 (exact in fp32)

__global__ __launch_bounds__(EM_T) void edge_metric_kernel(const uint8_t* __restrict__ e_op,
                                                           const uint8_t* __restrict__ e_gt, int h,
                                                           int w, double* __restrict__ out) {
  __shared__ long long red[4][EM_T / 64];
  const long hw = (long)h * w;
  const uint8_t* a = e_op + (long)blockIdx.x * hw;
  const uint8_t* b = e_gt + (long)blockIdx.x * hw;
  long long v[4] = {0, 0, 0, 0};  // sum of dt(gt) on op's edges, #op edges, sum dt(op) on gt's, #gt
  for (long i = threadIdx.x; i < hw; i += EM_T) {
    const bool ea = a[i] != 0, eb = b[i] != 0;
    v[1] += ea;
    v[3] += eb;
    if (ea && eb) {
      const int y = (int)(i / w), x = (int)(i % w);
      const int fb = chamfer_fixed(b, h, w, y, x, DT_MAX_RADIUS);
      const int fa = chamfer_fixed(a, h, w, y, x, DT_MAX_RADIUS);
      if (fb <= DT_CUT) v[0] += fb;
      if (fa <= DT_CUT) v[2] += fa;
    }
  }
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    long long s = v[k];
    for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o, 64);
    if (lane == 0) red[k][wave] = s;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    long long t[4] = {0, 0, 0, 0};
    for (int k = 0; k < 4; ++k)
      for (int j = 0; j < EM_T / 64; ++j) t[k] += red[k][j];
    out[2 * blockIdx.x] = ((double)t[0] / 65536.0) / (double)t[1];      // 0.0 / 0.0 = nan
    out[2 * blockIdx.x + 1] = ((double)t[2] / 65536.0) / (double)t[3];
  }
}

// workspace layout of the Canny entry points: [n][256] histogram, then the strong and the weak
// bit maps, [n][h][wpr] words each
inline int words_per_row(int w) { return 2 * (int)cdiv(w, NMS_TW); }

static int canny_launch(const uint8_t* img, int n, int h, int w, const int* thr, int lo, int hi,
                 uint8_t* edges, int* sweeps, void* ws, hipStream_t st) {
  const int wpr = words_per_row(w);
  unsigned* strong = (unsigned*)ws + (size_t)n * 256;
  unsigned* weak = strong + (size_t)n * h * wpr;
  canny_nms_kernel<<<dim3(cdiv(w, NMS_TW), cdiv(h, NMS_TH), n), NMS_T, 0, st>>>(
      img, h, w, thr, lo, hi, strong, weak);
  int rc = check_launch("canny_nms_kernel");
  if (rc) return rc;
  hysteresis_kernel<<<n, HYST_T, 0, st>>>(strong, weak, h, w, wpr, edges, sweeps);
  return check_launch("hysteresis_kernel");
}

}  // namespace pld

using namespace pld;

#define PLD_CHECK_EDGE_DIMS(who, h, w)                                                     \
  do {                                                                                     \
    if ((h) > PLD_EDGE_MAX_DIM || (w) > PLD_EDGE_MAX_DIM) {                                \
      ::pld::set_error("%s: %d x %d map above the %d x %d limit", who, (int)(h), (int)(w), \
                       PLD_EDGE_MAX_DIM, PLD_EDGE_MAX_DIM);                                \
      return PLD_ERR_UNSUPPORTED;                                                          \
    }                                                                                      \
  } while (0)

extern "C" size_t pld_minmax_u8_workspace_size(int n) {
  return n > 0 ? (size_t)n * MM_MAXB * 2 * sizeof(float) : 0;
}

extern "C" int pld_minmax_u8(const float* x, int n, int64_t hw, uint8_t* out, void* ws,
                             void* stream) {
  PLD_CHECK_ARG(x && out && ws && n > 0 && hw > 0, "pld_minmax_u8: bad args");
  const int nb = (int)std::min<long>(MM_MAXB, std::max<long>(1, (hw + 4095) / 4096));
  const long per = (hw + nb - 1) / nb;
  minmax_partial_kernel<<<dim3(nb, n), MM_T, 0, as_stream(stream)>>>(x, hw, per, (float*)ws);
  int rc = check_launch("minmax_partial_kernel");
  if (rc) return rc;
  minmax_map_kernel<<<dim3(nb, n), MM_T, 0, as_stream(stream)>>>(x, hw, per, (const float*)ws,
                                                                out);
  return check_launch("minmax_map_kernel");
}

extern "C" size_t pld_canny_workspace_size(int n, int h, int w) {
  if (n <= 0 || h <= 0 || w <= 0) return 0;
  return ((size_t)n * 256 + 2 * (size_t)n * h * words_per_row(w)) * sizeof(unsigned);
}

extern "C" int pld_canny_u8(const uint8_t* img, int n, int h, int w, int lo, int hi,
                            uint8_t* edges, int32_t* sweeps, void* ws, void* stream) {
  PLD_CHECK_ARG(img && edges && ws && n > 0 && h > 0 && w > 0, "pld_canny_u8: bad args");
  PLD_CHECK_EDGE_DIMS("pld_canny_u8", h, w);
  return canny_launch(img, n, h, w, nullptr, lo, hi, edges, sweeps, ws, as_stream(stream));
}

extern "C" int pld_auto_canny_u8(const uint8_t* img, int n, int h, int w, double lo_factor,
                                 double hi_factor, int32_t* thr_out, uint8_t* edges,
                                 int32_t* sweeps, void* ws, void* stream) {
  PLD_CHECK_ARG(img && thr_out && edges && ws && n > 0 && h > 0 && w > 0,
                "pld_auto_canny_u8: bad args");
  PLD_CHECK_EDGE_DIMS("pld_auto_canny_u8", h, w);
  hipStream_t st = as_stream(stream);
  const long hw = (long)h * w;
  unsigned* hist = (unsigned*)ws;
  hist_clear_kernel<<<n, HIST_T, 0, st>>>(hist, (long)n * 256);
  int rc = check_launch("hist_clear_kernel");
  if (rc) return rc;
  const int nb = (int)std::min<long>(HIST_MAXB, std::max<long>(1, (hw + 4095) / 4096));
  const long per = (hw + nb - 1) / nb;
  hist_kernel<<<dim3(nb, n), HIST_T, 0, st>>>(img, hw, per, hist);
  rc = check_launch("hist_kernel");
  if (rc) return rc;
  median_thresholds_kernel<<<cdiv(n, 64), 64, 0, st>>>(hist, n, hw, lo_factor, hi_factor, thr_out);
  rc = check_launch("median_thresholds_kernel");
  if (rc) return rc;
  return canny_launch(img, n, h, w, thr_out, 0, 0, edges, sweeps, ws, st);
}

extern "C" int pld_chamfer_dt3(const uint8_t* mask, int n, int h, int w, float max_dist,
                               float* out, void* stream) {
  PLD_CHECK_ARG(mask && out && n > 0 && h > 0 && w > 0 && max_dist >= 0.f,
                "pld_chamfer_dt3: bad args");
  // a distance of at most max_dist is at most this many steps away in rows and in columns
  const double steps = (double)max_dist * 65536.0 / HV_DIST;
  if (!(steps < DT_MAX_RADIUS + 1)) {
    set_error("pld_chamfer_dt3: max_dist %g needs a search radius above %d", (double)max_dist,
              DT_MAX_RADIUS);
    return PLD_ERR_UNSUPPORTED;
  }
  chamfer_dt3_kernel<<<dim3(cdiv((long)h * w, 256), n), 256, 0, as_stream(stream)>>>(
      mask, h, w, (int)steps, max_dist, out);
  return check_launch("chamfer_dt3_kernel");
}

extern "C" int pld_depth_edge_metric(const uint8_t* edges_op, const uint8_t* edges_gt, int n, int h,
                                     int w, double* out, void* stream) {
  PLD_CHECK_ARG(edges_op && edges_gt && out && n > 0 && h > 0 && w > 0,
                "pld_depth_edge_metric: bad args");
  edge_metric_kernel<<<n, EM_T, 0, as_stream(stream)>>>(edges_op, edges_gt, h, w, out);
  return check_launch("edge_metric_kernel");
}
