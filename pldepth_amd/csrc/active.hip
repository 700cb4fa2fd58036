// The active-learning round's selection pass (pldepth/run_scripts/active_PLDepth.py:160-185),
// batched over images on the GPU:
//   active_learning_data_provider   pldepth/active_learning/active_learning_method.py:79-119
//   active_sampling / get_edge_pixel  :12-56        oracle  :59-76
//   hausdorff_distance / hausdorff_pair   pldepth/active_learning/metrics.py:9-57
//   unsharp_mask                          pldepth/active_learning/preprocess_utils.py:16-26
// The OpenCV calls the reference makes on the way are restated here (unpinned, like the ones of
// edges.hip): cv2.cvtColor(RGB2GRAY) on float32, cv2.medianBlur on 8-bit maps, cv2.normalize to
// 0..255 as float32 and cv2.GaussianBlur((5, 5), sigma). Every float operation that decides a
// result rounds on its own (mul_rn / add_rn) and everything else is integer arithmetic, so every
// entry point equals the NumPy restatement (tests/al_ref.py) bit for bit, whatever the thread
// order.
#include <algorithm>
#include <cfloat>
#include <climits>
#include <cmath>

#include "common.h"

namespace pld {

// ---------------------------------------------------------------------------------------------
// RGB -> gray: (r * 0.299f + g * 0.587f) + b * 0.114f, every product and sum rounded on its own
// ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void gray_kernel(const float* __restrict__ rgb, long total,
                                                   float* __restrict__ gray) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= total) return;
  const float r = rgb[3 * i], g = rgb[3 * i + 1], b = rgb[3 * i + 2];
  gray[i] = add_rn(add_rn(mul_rn(r, 0.299f), mul_rn(g, 0.587f)), mul_rn(b, 0.114f));
}

// ---------------------------------------------------------------------------------------------
// Median of the ksize x ksize window (border replicated). One block per 32 x 8 tile: the tile
// with its halo goes to LDS, and every pixel finds its median bit by bit from the top: the median
// is the largest level v with #{window < v} <= ksize^2 / 2, and that count grows with v. The tile
// holds one pixel per LDS word: neighbouring lanes read neighbouring banks, and every read is
// aligned (byte pixels let the compiler fuse a window row into 16-byte reads at odd addresses).
// ---------------------------------------------------------------------------------------------
constexpr int MED_TW = 32, MED_TH = 8, MED_T = MED_TW * MED_TH;
constexpr int MED_MAX_R = PLD_MEDIAN_MAX_KSIZE / 2;

__global__ __launch_bounds__(MED_T) void median_blur_kernel(const uint8_t* __restrict__ img,
                                                            int h, int w, int rad,
                                                            uint8_t* __restrict__ out) {
  __shared__ int px[MED_TH + 2 * MED_MAX_R][MED_TW + 2 * MED_MAX_R];
  const uint8_t* p = img + (long)blockIdx.z * h * w;
  const int x0 = blockIdx.x * MED_TW, y0 = blockIdx.y * MED_TH;
  const int lw = MED_TW + 2 * rad, lh = MED_TH + 2 * rad;
  for (int i = threadIdx.x; i < lw * lh; i += MED_T) {
    const int ly = i / lw, lx = i % lw;
    const int y = min(max(y0 + ly - rad, 0), h - 1), x = min(max(x0 + lx - rad, 0), w - 1);
    px[ly][lx] = p[(long)y * w + x];
  }
  __syncthreads();
  const int lx = threadIdx.x % MED_TW, ly = threadIdx.x / MED_TW;
  const int x = x0 + lx, y = y0 + ly;
  if (x >= w || y >= h) return;
  const int k = 2 * rad + 1, half = (k * k) / 2;
  int med = 0;
  for (int bit = 128; bit > 0; bit >>= 1) {
    const int cand = med | bit;
    int below = 0;
    for (int dy = 0; dy < k; ++dy) {
#pragma clang loop vectorize(disable) unroll_count(5)
      for (int dx = 0; dx < k; ++dx) below += px[ly + dy][lx + dx] < cand;
    }
    if (below <= half) med = cand;
  }
  out[((long)blockIdx.z * h + y) * w + x] = (uint8_t)med;
}

// ---------------------------------------------------------------------------------------------
// unsharp_mask of the min-max scaled map. Two launches: per-block partial min / max of each image
// (the layout of edges.hip's minmax: [n][blocks][2] floats), then one block per 32 x 8 tile:
// f = (float)((double)x * scale + shift) for the tile and a 2-pixel ring (BORDER_REFLECT_101),
// the 5-tap row filter, the 5-tap column filter, (amount + 1) * f - amount * blur, clamp to
// [0, 255] and round half to even. Taps accumulate from the lowest index up.
// ---------------------------------------------------------------------------------------------
constexpr int US_T = 256;
constexpr int US_MAXB = 64;  // partials per image (workspace: n * US_MAXB * 2 floats)
constexpr int US_TW = 32, US_TH = 8;

__device__ __forceinline__ void wave_minmax(float& mn, float& mx) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    mn = fminf(mn, __shfl_xor(mn, o, 64));
    mx = fmaxf(mx, __shfl_xor(mx, o, 64));
  }
}

// min / max over the block's 4 waves, in every thread
__device__ __forceinline__ void block_minmax4(float& mn, float& mx, float (*red)[2]) {
  wave_minmax(mn, mx);
  if ((threadIdx.x & 63) == 0) {
    red[threadIdx.x >> 6][0] = mn;
    red[threadIdx.x >> 6][1] = mx;
  }
  __syncthreads();
  mn = fminf(fminf(red[0][0], red[1][0]), fminf(red[2][0], red[3][0]));
  mx = fmaxf(fmaxf(red[0][1], red[1][1]), fmaxf(red[2][1], red[3][1]));
}

__global__ __launch_bounds__(US_T) void unsharp_partial_kernel(const float* __restrict__ x,
                                                               long hw, long per,
                                                               float* __restrict__ part) {
  __shared__ float red[4][2];
  const float* p = x + (long)blockIdx.y * hw;
  const long i0 = (long)blockIdx.x * per;
  const long i1 = i0 + per < hw ? i0 + per : hw;
  float mn = FLT_MAX, mx = -FLT_MAX;
  for (long i = i0 + threadIdx.x; i < i1; i += US_T) {
    const float v = p[i];
    mn = fminf(mn, v);
    mx = fmaxf(mx, v);
  }
  block_minmax4(mn, mx, red);
  if (threadIdx.x == 0) {
    float* o = part + ((long)blockIdx.y * gridDim.x + blockIdx.x) * 2;
    o[0] = mn;
    o[1] = mx;
  }
}

__device__ __forceinline__ int reflect101(int i, int n) {
  if (n == 1) return 0;
  while (i < 0 || i >= n) i = i < 0 ? -i : 2 * n - 2 - i;
  return i;
}

struct Taps5 {
  float w[5];
};

__device__ __forceinline__ float scale_shift_f32(float v, double scale, double shift) {
#pragma clang fp contract(off)
  const double t = (double)v * scale;
  return (float)(t + shift);
}

__global__ __launch_bounds__(US_T) void unsharp_kernel(const float* __restrict__ x, int h, int w,
                                                       const float* __restrict__ part, int nparts,
                                                       int normalize, Taps5 taps, float amount1,
                                                       float amount,
                                                       uint8_t* __restrict__ out) {
  __shared__ float red[4][2];
  __shared__ float src[US_TH + 4][US_TW + 4];
  __shared__ float rowb[US_TH + 4][US_TW];
  const int im = blockIdx.z;
  const float* pp = part + (long)im * nparts * 2;
  float mn = FLT_MAX, mx = -FLT_MAX;
  if (normalize && (int)threadIdx.x < nparts) {
    mn = pp[2 * threadIdx.x];
    mx = pp[2 * threadIdx.x + 1];
  }
  block_minmax4(mn, mx, red);
  const double smin = mn, smax = mx;
  // normalize == 0: the map is taken as it is ((double)x * 1 + 0 is x)
  double scale = 1.0, shift = 0.0;
  if (normalize) {
    scale = (smax - smin) > DBL_EPSILON ? 255.0 / (smax - smin) : 0.0;
    shift = -smin * scale;
  }
  const float* p = x + (long)im * h * w;
  const int x0 = blockIdx.x * US_TW, y0 = blockIdx.y * US_TH;
  for (int i = threadIdx.x; i < (US_TH + 4) * (US_TW + 4); i += US_T) {
    const int ly = i / (US_TW + 4), lx = i % (US_TW + 4);
    // rows and columns past the image feed only outputs that are not written
    const int yy = reflect101(min(y0 + ly - 2, h + 1), h);
    const int xx = reflect101(min(x0 + lx - 2, w + 1), w);
    src[ly][lx] = scale_shift_f32(p[(long)yy * w + xx], scale, shift);
  }
  __syncthreads();
  for (int i = threadIdx.x; i < (US_TH + 4) * US_TW; i += US_T) {
    const int ly = i / US_TW, lx = i % US_TW;
    float acc = mul_rn(src[ly][lx], taps.w[0]);
#pragma unroll
    for (int k = 1; k < 5; ++k) acc = add_rn(acc, mul_rn(src[ly][lx + k], taps.w[k]));
    rowb[ly][lx] = acc;
  }
  __syncthreads();
  const int lx = threadIdx.x % US_TW, ly = threadIdx.x / US_TW;
  const int xo = x0 + lx, yo = y0 + ly;
  if (xo >= w || yo >= h) return;
  float blur = mul_rn(rowb[ly][lx], taps.w[0]);
#pragma unroll
  for (int k = 1; k < 5; ++k) blur = add_rn(blur, mul_rn(rowb[ly + k][lx], taps.w[k]));
  const float f = src[ly + 2][lx + 2];
  const float s = add_rn(mul_rn(amount1, f), -mul_rn(amount, blur));
  const float c = s > 0.f ? (s < 255.f ? s : 255.f) : 0.f;  // NaN -> 0
  out[((long)im * h + yo) * w + xo] = (uint8_t)(int)rintf(c);
}

// ---------------------------------------------------------------------------------------------
// Tiles of at most 32 x 32 pixels as row bit masks (bit c of word r = pixel (r, c) is non-zero),
// one 64-lane wave per tile and AL_WAVES tiles per workgroup. Two rows are read per step (lanes
// 0-31 one row, lanes 32-63 the next) and their ballot is the two row words.
// ---------------------------------------------------------------------------------------------
constexpr int AL_WAVES = 4, AL_T = 64 * AL_WAVES;

__device__ __forceinline__ void load_tile_rows(const uint8_t* __restrict__ tile, int w, int t,
                                               int lane, unsigned* rows) {
  for (int r0 = 0; r0 < PLD_TILE_MAX; r0 += 2) {
    const int r = r0 + (lane >> 5), c = lane & 31;
    const bool on = r < t && c < t && tile[(long)r * w + c] != 0;
    const unsigned long long b = __ballot(on);
    if (lane == 0) {
      rows[r0] = (unsigned)b;
      rows[r0 + 1] = (unsigned)(b >> 32);
    }
  }
}

// origin of tile `tile` (row-major over the image's split x split tiles, images one after another)
__device__ __forceinline__ const uint8_t* tile_origin(const uint8_t* __restrict__ maps, int tile,
                                                      int h, int w, int split, int t) {
  const int per = split * split;
  const int im = tile / per, ti = tile % per;
  return maps + ((long)im * h + (long)(ti / split) * t) * w + (long)(ti % split) * t;
}

// The set pixel of rows[0..t) nearest to (r, c) as (d2 << 10) | (r2 * 32 + c2): the minimum over
// the rows of the nearest set bit at or below column c (clz) and at or above it (ctz), so equal
// distances resolve to the lowest row-major index. INT_MAX for an empty set.
__device__ __forceinline__ int nearest_key(const unsigned* rows, int t, int r, int c) {
  int best = INT_MAX;
  for (int r2 = 0; r2 < t; ++r2) {
    const unsigned wd = rows[r2];
    if (!wd) continue;
    const int dy2 = (r2 - r) * (r2 - r);
    const unsigned lo = wd & (0xffffffffu >> (31 - c)), hi = wd >> c;
    if (lo) {
      const int c2 = 31 - __builtin_clz(lo);
      best = min(best, ((dy2 + (c - c2) * (c - c2)) << 10) | (r2 * 32 + c2));
    }
    if (hi) {
      const int dx = __builtin_ctz(hi);
      best = min(best, ((dy2 + dx * dx) << 10) | (r2 * 32 + c + dx));
    }
  }
  return best;
}

// max over the pixels p of `from` of the squared distance to the nearest pixel q of `to`, as
// (d2 << 20) | ((1023 - p) << 10) | q with p, q = row * 32 + column: the integer maximum is the
// first p in row-major order that attains the distance, together with its nearest q. Both sets
// hold a pixel. d2 <= 2 * 31^2 < 2^11, so the key is a positive int.
__device__ __forceinline__ int directed_key(const unsigned* from, const unsigned* to, int t,
                                            int lane) {
  int best = -1;
  for (int i = lane; i < t * 32; i += 64) {
    const int r = i >> 5, c = i & 31;
    if (!((from[r] >> c) & 1u)) continue;
    const int nk = nearest_key(to, t, r, c);
    best = max(best, ((nk >> 10) << 20) | ((1023 - i) << 10) | (nk & 1023));
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) best = max(best, __shfl_xor(best, o, 64));
  return best;
}

__global__ __launch_bounds__(AL_T) void tile_hausdorff_kernel(const uint8_t* __restrict__ e_in,
                                                              const uint8_t* __restrict__ e_pred,
                                                              int ntiles, int h, int w, int split,
                                                              int t, int* __restrict__ out) {
  __shared__ unsigned rows[AL_WAVES][2][PLD_TILE_MAX];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int tile = blockIdx.x * AL_WAVES + wave;
  const bool live = tile < ntiles;
  unsigned* A = rows[wave][0];
  unsigned* B = rows[wave][1];
  if (live) {
    load_tile_rows(tile_origin(e_in, tile, h, w, split, t), w, t, lane, A);
    load_tile_rows(tile_origin(e_pred, tile, h, w, split, t), w, t, lane, B);
  }
  __syncthreads();
  if (!live) return;
  int na = 0, nb = 0;
  for (int r = 0; r < t; ++r) {
    na += __popc(A[r]);
    nb += __popc(B[r]);
  }
  int res[8] = {0, -1, -1, -1, -1, na, nb, -1};
  if (na == 0 || nb == 0) {
    res[0] = (na == 0 && nb == 0) ? 0 : -1;
  } else {
    const int kab = directed_key(A, B, t, lane), kba = directed_key(B, A, t, lane);
    const int hab = kab >> 20, hba = kba >> 20;
    const int br = hab > hba;
    const int k = br ? kab : kba;
    const int first = 1023 - ((k >> 10) & 1023), near = k & 1023;
    const int pin = br ? first : near, ppred = br ? near : first;
    res[0] = max(hab, hba);
    res[1] = pin >> 5;
    res[2] = pin & 31;
    res[3] = ppred >> 5;
    res[4] = ppred & 31;
    res[7] = br;
  }
  if (lane < 8) {
    int v = res[0];
#pragma unroll
    for (int j = 1; j < 8; ++j) v = lane == j ? res[j] : v;
    out[(long)tile * 8 + lane] = v;
  }
}

__global__ __launch_bounds__(AL_T) void tile_nth_edge_kernel(const uint8_t* __restrict__ e_in,
                                                             int ntiles, int h, int w, int split,
                                                             int t, const int* __restrict__ ks,
                                                             int* __restrict__ rc) {
  __shared__ unsigned rows[AL_WAVES][PLD_TILE_MAX];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int tile = blockIdx.x * AL_WAVES + wave;
  const int k = tile < ntiles ? ks[tile] : -1;  // the same in every lane of the wave
  if (k >= 0) load_tile_rows(tile_origin(e_in, tile, h, w, split, t), w, t, lane, rows[wave]);
  __syncthreads();
  if (k < 0 || lane != 0) return;
  int r_out = -1, c_out = -1, seen = 0;
  for (int r = 0; r < t; ++r) {
    unsigned wd = rows[wave][r];
    const int pc = __popc(wd);
    if (k < seen + pc) {
      for (int j = k - seen; j > 0; --j) wd &= wd - 1;  // drop the j lowest set bits
      r_out = r;
      c_out = __builtin_ctz(wd);
      break;
    }
    seen += pc;
  }
  rc[2 * (long)tile] = r_out;
  rc[2 * (long)tile + 1] = c_out;
}

// ---------------------------------------------------------------------------------------------
// oracle (active_learning_method.py:59-76): one thread per output row. Row j < P / L takes the
// points j L .. j L + L - 1 when j L < P - L (the reference's loop bound) and stays zero
// otherwise; its entries (r * row_stride + c, gt[r][c]) are ordered by depth descending, equal
// depths by later list position first (np.argsort(...)[::-1] with a stable ascending sort).
// A point outside the map reads no memory and ranks with depth 0.
// ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(64) void al_oracle_kernel(const float* __restrict__ gt, int n, int h,
                                                       int w, const int* __restrict__ pos_xy,
                                                       int P, int L, int row_stride,
                                                       float* __restrict__ out) {
  const int rows = P / L;
  const long id = (long)blockIdx.x * 64 + threadIdx.x;
  if (id >= (long)n * rows) return;
  const int im = (int)(id / rows), j = (int)(id % rows);
  float* o = out + id * L * 2;
  if (j * L >= P - L) {
    for (int k = 0; k < 2 * L; ++k) o[k] = 0.f;
    return;
  }
  const int* pts = pos_xy + ((long)im * P + (long)j * L) * 2;
  const float* g = gt + (long)im * h * w;
  float pos[PLD_ORACLE_MAX_L], dep[PLD_ORACLE_MAX_L];
  for (int k = 0; k < L; ++k) {
    const int r = pts[2 * k], c = pts[2 * k + 1];
    const float p = (float)(unsigned)(r * row_stride + c);
    const float d = (r >= 0 && r < h && c >= 0 && c < w) ? g[(long)r * w + c] : 0.f;
    // insertion from the back: the new (latest) entry moves in front of every entry that is not
    // deeper than it
    int i = k;
    while (i > 0 && !(dep[i - 1] > d)) {
      dep[i] = dep[i - 1];
      pos[i] = pos[i - 1];
      --i;
    }
    dep[i] = d;
    pos[i] = p;
  }
  for (int k = 0; k < L; ++k) {
    o[2 * k] = pos[k];
    o[2 * k + 1] = dep[k];
  }
}

static int check_tiles(const char* who, int h, int w, int split) {
  if (h != w || h % split != 0 || h / split > PLD_TILE_MAX) {
    set_error("%s: %d x %d map in %d x %d tiles: the map must be square, divide evenly and give "
              "tiles of at most %d x %d pixels", who, h, w, split, split, PLD_TILE_MAX,
              PLD_TILE_MAX);
    return PLD_ERR_UNSUPPORTED;
  }
  return PLD_OK;
}

}  // namespace pld

using namespace pld;

extern "C" int pld_gray_f32(const float* rgb, int n, int64_t hw, float* gray, void* stream) {
  PLD_CHECK_ARG(rgb && gray && n > 0 && hw > 0, "pld_gray_f32: bad args");
  const long total = (long)n * hw;
  gray_kernel<<<cdiv(total, 256), 256, 0, as_stream(stream)>>>(rgb, total, gray);
  return check_launch("gray_kernel");
}

extern "C" int pld_median_blur_u8(const uint8_t* img, int n, int h, int w, int ksize,
                                  uint8_t* out, void* stream) {
  PLD_CHECK_ARG(img && out && n > 0 && h > 0 && w > 0 && ksize >= 3 && (ksize & 1),
                "pld_median_blur_u8: bad args");
  if (ksize > PLD_MEDIAN_MAX_KSIZE) {
    set_error("pld_median_blur_u8: ksize %d above the limit of %d", ksize, PLD_MEDIAN_MAX_KSIZE);
    return PLD_ERR_UNSUPPORTED;
  }
  median_blur_kernel<<<dim3(cdiv(w, MED_TW), cdiv(h, MED_TH), n), MED_T, 0, as_stream(stream)>>>(
      img, h, w, ksize / 2, out);
  return check_launch("median_blur_kernel");
}

extern "C" size_t pld_unsharp_u8_workspace_size(int n) {
  return n > 0 ? (size_t)n * US_MAXB * 2 * sizeof(float) : 0;
}

extern "C" int pld_unsharp_u8(const float* x, int n, int h, int w, int normalize, float sigma,
                              float amount, uint8_t* out, void* ws, void* stream) {
  PLD_CHECK_ARG(x && out && (ws || !normalize) && n > 0 && h > 0 && w > 0 && sigma > 0.f,
                "pld_unsharp_u8: bad args");
  const long hw = (long)h * w;
  const int nb = (int)std::min<long>(US_MAXB, std::max<long>(1, (hw + 4095) / 4096));
  const long per = (hw + nb - 1) / nb;
  hipStream_t st = as_stream(stream);
  if (normalize) {
    unsharp_partial_kernel<<<dim3(nb, n), US_T, 0, st>>>(x, hw, per, (float*)ws);
    int rc = check_launch("unsharp_partial_kernel");
    if (rc) return rc;
  }
  Taps5 taps;
  double g[5], sum = 0.0;
  for (int k = 0; k < 5; ++k) {
    const double d = k - 2;
    g[k] = std::exp(-(d * d) / (2.0 * (double)sigma * (double)sigma));
    sum += g[k];
  }
  for (int k = 0; k < 5; ++k) taps.w[k] = (float)(g[k] / sum);
  unsharp_kernel<<<dim3(cdiv(w, US_TW), cdiv(h, US_TH), n), US_T, 0, st>>>(
      x, h, w, (const float*)ws, nb, normalize, taps, (float)((double)amount + 1.0), amount, out);
  return check_launch("unsharp_kernel");
}

extern "C" int pld_tile_hausdorff(const uint8_t* edges_in, const uint8_t* edges_pred, int n, int h,
                                  int w, int split, int32_t* out, void* stream) {
  PLD_CHECK_ARG(edges_in && edges_pred && out && n > 0 && h > 0 && w > 0 && split > 0,
                "pld_tile_hausdorff: bad args");
  int rc = check_tiles("pld_tile_hausdorff", h, w, split);
  if (rc) return rc;
  const long ntiles = (long)n * split * split;
  PLD_CHECK_ARG(ntiles <= INT_MAX / 8, "pld_tile_hausdorff: too many tiles");
  tile_hausdorff_kernel<<<cdiv(ntiles, AL_WAVES), AL_T, 0, as_stream(stream)>>>(
      edges_in, edges_pred, (int)ntiles, h, w, split, h / split, out);
  return check_launch("tile_hausdorff_kernel");
}

extern "C" int pld_tile_nth_edge(const uint8_t* edges_in, int n, int h, int w, int split,
                                 const int32_t* k, int32_t* rc_out, void* stream) {
  PLD_CHECK_ARG(edges_in && k && rc_out && n > 0 && h > 0 && w > 0 && split > 0,
                "pld_tile_nth_edge: bad args");
  int rc = check_tiles("pld_tile_nth_edge", h, w, split);
  if (rc) return rc;
  const long ntiles = (long)n * split * split;
  PLD_CHECK_ARG(ntiles <= INT_MAX / 8, "pld_tile_nth_edge: too many tiles");
  tile_nth_edge_kernel<<<cdiv(ntiles, AL_WAVES), AL_T, 0, as_stream(stream)>>>(
      edges_in, (int)ntiles, h, w, split, h / split, k, rc_out);
  return check_launch("tile_nth_edge_kernel");
}

extern "C" int pld_al_oracle(const float* gt, int n, int h, int w, const int32_t* pos_xy, int P,
                             int L, int row_stride, float* out, void* stream) {
  PLD_CHECK_ARG(gt && pos_xy && out && n > 0 && h > 0 && w > 0 && P > 0 && L > 0 &&
                    row_stride > 0,
                "pld_al_oracle: bad args");
  if (L > PLD_ORACLE_MAX_L) {
    set_error("pld_al_oracle: ranking size %d above the limit of %d", L, PLD_ORACLE_MAX_L);
    return PLD_ERR_UNSUPPORTED;
  }
  const long rows = (long)n * (P / L);
  if (rows == 0) return PLD_OK;  // fewer points than one ranking: the result is empty
  al_oracle_kernel<<<cdiv(rows, 64), 64, 0, as_stream(stream)>>>(gt, n, h, w, pos_xy, P, L,
                                                                 row_stride, out);
  return check_launch("al_oracle_kernel");
}
