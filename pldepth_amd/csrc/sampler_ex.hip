// Ranking sampler with the strategy classes' arguments as run-time values: pld_sampler_rank_ex
// (and pld_sampler_minmax), beside pld_sampler_rank (sampler.hip), which keeps the reference's
// defaults as constants and is left as it is.
//   tau, penalty : `threshold` / `equality_penalty` of Thresholded and Info (sampling.py:179-188,
//                  212-216); the bounds float32(1 + tau), float32(1 / (1 + tau)) are formed in
//                  double on the host, as NumPy (NEP 50) casts the Python floats
//   n_cand       : int(R * batch_size_factor), formed by the caller (sampling.py:55)
//   mask grid    : a consistency mask of another resolution than the image: valid_idx holds
//                  positions of the mask grid, mapped to pixels as sampling.py:115-116,125-129
//   RANDOM       : RandomSamplingStrategy.sample_points_batch (sampling.py:89-103): draws are
//                  pixels, lists keep their draw order, float64 gap-sum score (:34-42)
// The kernels are sampler.hip's candidate / selection kernels with those values read from the
// parameter block, in the same float types and operation order (bit-exact against
// tests/sampler_params_ref.py, and against pld_sampler_rank at the defaults). They are a second
// copy rather than shared code so that pld_sampler_rank's kernels stay untouched.
// Compiled with -ffp-contract=off: no FMA contraction may change a rounding step.
#include <algorithm>
#include <cmath>

#include "common.h"

namespace pld {
namespace sampler_ex {

constexpr int MINMAX_THREADS = 1024;

// ------------------------------------------------------------------ per-list sort + score
// NumPy float32 add.reduce of a contiguous array: 0 + pairwise_sum (oracle.sampler.pairwise_sum32)
__device__ float pairwise_sum32(const float* a, int n) {
  // iterative form of the recursion: the recursion only splits when n > 128
  if (n < 8) {
    float res = -0.0f;
    for (int i = 0; i < n; ++i) res = add_rn(res, a[i]);
    return res;
  }
  if (n <= 128) {
    float r[8];
    for (int j = 0; j < 8; ++j) r[j] = a[j];
    int i = 8;
    for (; i < n - (n % 8); i += 8)
      for (int j = 0; j < 8; ++j) r[j] = add_rn(r[j], a[i + j]);
    float res = add_rn(add_rn(r[0], r[1]), add_rn(r[2], r[3]));
    res = add_rn(res, add_rn(add_rn(r[4], r[5]), add_rn(r[6], r[7])));
    for (; i < n; ++i) res = add_rn(res, a[i]);
    return res;
  }
  int n2 = n / 2;
  n2 -= n2 % 8;
  return add_rn(pairwise_sum32(a, n2), pairwise_sum32(a + n2, n - n2));
}

__device__ float pairwise_sum32_top(const float* a, int n) {
  return add_rn(0.0f, pairwise_sum32(a, n));
}

struct RankParams {
  const float* gt;
  const int* valid_idx;
  const int* nvalid;
  const float* gt_minmax;
  const int* draws;
  int B, H, W, L, n_cand, R_out, strategy;
  float* cand;     // [B][n_cand][L][2]
  double* score;   // [B][n_cand]
  float* out;      // [B][R_out][L][2]
};

// the classes' arguments; RankParams alone is what the selection kernels read
struct RankParamsEx : RankParams {
  // get_depth_relation's bounds float32(1 + tau), float32(1 / (1 + tau)) (depth_utils.py:16-18)
  // and the equality penalty as Thresholded (float32) and Info (float64) accumulate it
  float hi, lo, pen32;
  double pen64;
  // the mask's grid: valid_idx holds flat positions of it, mask_hw per image; scaled != 0 when
  // it is not the image's, a position then maps through xs = H / mask_h, ys = W / mask_w
  int mask_w, mask_hw, scaled;
  double xs, ys;
};

// what the candidate kernels read through (sampler.hip's have these as constants)
__device__ __forceinline__ float tau_hi(const RankParamsEx& p) { return p.hi; }
__device__ __forceinline__ float tau_lo(const RankParamsEx& p) { return p.lo; }
__device__ __forceinline__ float penalty32(const RankParamsEx& p) { return p.pen32; }
__device__ __forceinline__ double penalty64(const RankParamsEx& p) { return p.pen64; }
__device__ __forceinline__ bool unmasked(const RankParamsEx& p) {
  return p.strategy == PLD_SAMPLER_RANDOM;
}
__device__ __forceinline__ int valid_count(const RankParamsEx& p, int b) {
  return p.nvalid ? p.nvalid[b] : p.H * p.W;
}
// the image pixel (flat row*W+col) of draw d of image b, nv > 0 valid positions. Unmasked
// (valid_idx null): the draw is the pixel. Scaled mask: int(np.int64 * float), truncation toward
// zero (sampling.py:115-116), clamped to the image.
__device__ __forceinline__ int draw_pixel(const RankParamsEx& p, int b, int nv, int d) {
  d = min(max(d, 0), nv - 1);
  int pos = p.valid_idx ? p.valid_idx[(long)b * p.mask_hw + d] : d;
  if (p.scaled) {
    const int mr = pos / p.mask_w, mc = pos - mr * p.mask_w;
    const int row = min(max((int)((double)mr * p.xs), 0), p.H - 1);
    const int col = min(max((int)((double)mc * p.ys), 0), p.W - 1);
    pos = row * p.W + col;
  }
  return pos;
}

template <int LMAX, class Params>
__global__ __launch_bounds__(256) void candidate_kernel(Params p) {
  const long total = (long)p.B * p.n_cand;
  const int L = p.L;
  const int HW = p.H * p.W;
  for (long e = (long)blockIdx.x * blockDim.x + threadIdx.x; e < total;
       e += (long)gridDim.x * blockDim.x) {
    const int b = (int)(e / p.n_cand);
    const int* dr = p.draws + e * L;
    const float* gb = p.gt + (long)b * HW;
    const int nv = valid_count(p, b);
    float g[LMAX];
    int id[LMAX];
    for (int j = 0; j < L; ++j) {
      if (nv <= 0) {  // empty mask: nothing was compacted; a defined, all-invalid list (label
        id[j] = 0;    // -1: ListMLE's validity mask), never a read of the unwritten valid_idx
        g[j] = -1.0f;
        continue;
      }
      const int pos = draw_pixel(p, b, nv, dr[j]);
      id[j] = pos;
      g[j] = gb[pos];
    }
    float* c = p.cand + e * L * 2;
    if (unmasked(p))  // the unmasked list keeps its draw order (:98-99)
      for (int j = 0; j < L; ++j) {
        c[2 * j] = (float)id[j];
        c[2 * j + 1] = g[j];
      }
    // stable ascending insertion sort by g (then read reversed: descending, ties later-first)
    for (int i = 1; i < L; ++i) {
      const float kg = g[i];
      const int kid = id[i];
      int j = i - 1;
      while (j >= 0 && g[j] > kg) {
        g[j + 1] = g[j];
        id[j + 1] = id[j];
        --j;
      }
      g[j + 1] = kg;
      id[j + 1] = kid;
    }
    // descending copy in place (reverse)
    for (int i = 0, j = L - 1; i < j; ++i, --j) {
      const float tg = g[i]; g[i] = g[j]; g[j] = tg;
      const int ti = id[i]; id[i] = id[j]; id[j] = ti;
    }
    if (!unmasked(p))
      for (int j = 0; j < L; ++j) {
        c[2 * j] = (float)id[j];
        c[2 * j + 1] = g[j];
      }
    double sc = 0.0;
    if (p.strategy == PLD_SAMPLER_MASKED || p.strategy == PLD_SAMPLER_THRESH) {
      float acc = 0.0f;
      for (int j = 0; j + 1 < L; ++j) {
        if (p.strategy == PLD_SAMPLER_THRESH &&
            depth_relation32(g[j], g[j + 1], tau_hi(p), tau_lo(p)) == 0)
          acc = add_rn(acc, penalty32(p));
        acc = add_rn(acc, fabsf(__fsub_rn(g[j], g[j + 1])));
      }
      sc = (double)acc;
    } else if (unmasked(p)) {
      // calculate_depth_differences (sampling.py:34-42) on the float64 gts_buffer
      for (int j = 0; j + 1 < L; ++j)
        sc = __dadd_rn(sc, fabs(__dsub_rn((double)g[j], (double)g[j + 1])));
    } else if (p.strategy == PLD_SAMPLER_INFO) {
      // expected = np.linspace(min+0.001, max, L+1)[1:] in float32
      const float start = add_rn(p.gt_minmax[2 * b], 0.001f);
      const float stop = p.gt_minmax[2 * b + 1];
      const float delta = __fsub_rn(stop, start);
      const float stepv = __fdiv_rn(delta, (float)L);
      float t[LMAX];
      for (int j = 0; j < L; ++j) {
        const float ev = (j == L - 1) ? stop : add_rn(mul_rn((float)(j + 1), stepv), start);
        const float d = __fsub_rn(g[j], ev);
        t[j] = __fdiv_rn(mul_rn(d, d), ev);
      }
      sc = -(double)pairwise_sum32_top(t, L);
      for (int j = 0; j + 1 < L; ++j)
        if (depth_relation32(g[j], g[j + 1], tau_hi(p), tau_lo(p)) == 0)
          sc = __dadd_rn(sc, penalty64(p));
    }
    p.score[e] = sc;
  }
}

// 8 < L <= 64: one wavefront per candidate list, lane j holding draw j. The sort is a rank
// computation — position of j = #{k : g_k > g_j} + #{k : g_k == g_j, k > j}, exactly the
// stable-ascending-then-reversed order of candidate_kernel — and ds_permute moves each element to
// the lane of its position. Scores use the same fp32/fp64 operation order as candidate_kernel
// (NumPy's 8-accumulator pairwise sum for 8 <= L <= 128), computed redundantly by every lane.
template <class Params>
__global__ __launch_bounds__(256) void candidate_wave_kernel(Params p) {
  const int lane = threadIdx.x & 63;
  const long total = (long)p.B * p.n_cand;
  const int L = p.L;
  const int HW = p.H * p.W;
  for (long e = (long)blockIdx.x * 4 + (threadIdx.x >> 6); e < total; e += (long)gridDim.x * 4) {
    const int b = (int)(e / p.n_cand);
    float g = 0.0f;
    int id = 0;
    if (lane < L) {
      const int nv = valid_count(p, b);
      if (nv > 0) {
        id = draw_pixel(p, b, nv, p.draws[e * L + lane]);
        g = p.gt[(long)b * HW + id];
      } else {  // empty mask: defined all-invalid list (see candidate_kernel)
        g = -1.0f;
      }
    }
    const bool keep_order = unmasked(p);  // the unmasked list keeps its draw order (:98-99)
    int rank = 0;
    for (int k = 0; k < L; ++k) {  // wave-uniform trip count: every lane takes part in the shfl
      const float gk = __shfl(g, k, 64);
      rank += (gk > g) | ((gk == g) & (k > lane));
    }
    if (lane >= L) rank = lane;  // idle lanes keep their slot: the permutation stays 1:1
    const float gs = __int_as_float(__builtin_amdgcn_ds_permute(rank << 2, __float_as_int(g)));
    const int ids = __builtin_amdgcn_ds_permute(rank << 2, id);
    if (lane < L)
      reinterpret_cast<float2*>(p.cand + e * L * 2)[lane] =
          keep_order ? make_float2((float)id, g) : make_float2((float)ids, gs);
    double sc = 0.0;
    if (p.strategy == PLD_SAMPLER_MASKED || p.strategy == PLD_SAMPLER_THRESH) {
      float acc = 0.0f;
      float gj = __shfl(gs, 0, 64);
      for (int j = 0; j + 1 < L; ++j) {
        const float gj1 = __shfl(gs, j + 1, 64);
        if (p.strategy == PLD_SAMPLER_THRESH &&
            depth_relation32(gj, gj1, tau_hi(p), tau_lo(p)) == 0)
          acc = add_rn(acc, penalty32(p));
        acc = add_rn(acc, fabsf(__fsub_rn(gj, gj1)));
        gj = gj1;
      }
      sc = (double)acc;
    } else if (keep_order) {  // calculate_depth_differences, float64 (see candidate_kernel)
      float gj = __shfl(gs, 0, 64);
      for (int j = 0; j + 1 < L; ++j) {  // wave-uniform trip count, as above
        const float gj1 = __shfl(gs, j + 1, 64);
        sc = __dadd_rn(sc, fabs(__dsub_rn((double)gj, (double)gj1)));
        gj = gj1;
      }
    } else if (p.strategy == PLD_SAMPLER_INFO) {
      const float start = add_rn(p.gt_minmax[2 * b], 0.001f);
      const float stop = p.gt_minmax[2 * b + 1];
      const float stepv = __fdiv_rn(__fsub_rn(stop, start), (float)L);
      const float ev =
          (lane == L - 1) ? stop : add_rn(mul_rn((float)(lane + 1), stepv), start);
      const float dd = __fsub_rn(gs, ev);
      const float t = __fdiv_rn(mul_rn(dd, dd), ev);
      // pairwise_sum32, 8 <= n <= 128 branch
      float r[8];
#pragma unroll
      for (int j = 0; j < 8; ++j) r[j] = __shfl(t, j, 64);
      const int nfull = L - (L % 8);
      int i = 8;
      for (; i < nfull; i += 8)
#pragma unroll
        for (int j = 0; j < 8; ++j) r[j] = add_rn(r[j], __shfl(t, i + j, 64));
      float res = add_rn(add_rn(r[0], r[1]), add_rn(r[2], r[3]));
      res = add_rn(res, add_rn(add_rn(r[4], r[5]), add_rn(r[6], r[7])));
      for (; i < L; ++i) res = add_rn(res, __shfl(t, i, 64));
      sc = -(double)add_rn(0.0f, res);
      const float gn = __shfl(gs, min(lane + 1, 63), 64);
      const int nz =
          __popcll(__ballot(lane + 1 < L && depth_relation32(gs, gn, tau_hi(p), tau_lo(p)) == 0));
      for (int k = 0; k < nz; ++k) sc = __dadd_rn(sc, penalty64(p));
    }
    if (lane == 0) p.score[e] = sc;
  }
}

// per-image top-R, spread over (B, n / 256) workgroups: every workgroup stages the image's n
// scores in LDS and ranks 256 candidates against them, then copies the selected lists with all
// threads (coalesced). Same rank definition as select_kernel.
__global__ __launch_bounds__(256) void select_chunk_kernel(RankParams p) {
  extern __shared__ double s_score[];
  __shared__ int s_rank[256];
  const int b = blockIdx.x;
  const int n = p.n_cand;
  const double* sb = p.score + (long)b * n;
  for (int i = threadIdx.x; i < n; i += 256) s_score[i] = sb[i];
  __syncthreads();
  const int i = blockIdx.y * 256 + threadIdx.x;
  int rank = n;
  if (i < n) {
    const double si = s_score[i];
    int r0 = 0, r1 = 0;
    int j = 0;
    for (; j + 1 < n; j += 2) {
      const double s0 = s_score[j], s1 = s_score[j + 1];
      r0 += (s0 > si) | ((s0 == si) & (j > i));
      r1 += (s1 > si) | ((s1 == si) & (j + 1 > i));
    }
    if (j < n) r0 += (s_score[j] > si) | ((s_score[j] == si) & (j > i));
    rank = r0 + r1;
  }
  s_rank[threadIdx.x] = rank;
  __syncthreads();
  const int L2 = 2 * p.L;
  const int cnt = min(256, n - (int)blockIdx.y * 256);
  for (int q = threadIdx.x; q < cnt * L2; q += 256) {
    const int c = q / L2, k = q - c * L2;
    const int rk = s_rank[c];
    if (rk < p.R_out)
      p.out[((long)b * p.R_out + rk) * L2 + k] =
          p.cand[((long)b * n + blockIdx.y * 256 + c) * L2 + k];
  }
}

// per-image top-R: rank of candidate i = #{j : (score_j, j) > (score_i, i)} (lexicographic);
// the reference's argsort(scores)[::-1] order with ties broken toward the higher index
__global__ __launch_bounds__(1024) void select_kernel(RankParams p) {
  extern __shared__ double s_score[];
  const int b = blockIdx.x;
  const int n = p.n_cand;
  const double* sb = p.score + (long)b * n;
  for (int i = threadIdx.x; i < n; i += blockDim.x) s_score[i] = sb[i];
  __syncthreads();
  const int L = p.L;
  for (int i = threadIdx.x; i < n; i += blockDim.x) {
    const double si = s_score[i];
    int rank = 0;
    for (int j = 0; j < n; ++j) {
      const double sj = s_score[j];
      rank += (sj > si) | ((sj == si) & (j > i));
    }
    if (rank < p.R_out) {
      const float* src = p.cand + ((long)b * n + i) * L * 2;
      float* dst = p.out + ((long)b * p.R_out + rank) * L * 2;
      for (int k = 0; k < 2 * L; ++k) dst[k] = src[k];
    }
  }
}

// np.amin(gt), np.amax(gt) of whole images (sampling.py:219-220), one workgroup per image: the
// Info strategy's bounds when the mask's grid is not the image's (sampler.hip's compact_count_kernel
// gives them when it is, with the same fminf / fmaxf)
__global__ __launch_bounds__(MINMAX_THREADS) void minmax_kernel(const float* __restrict__ gt,
                                                                 int HW,
                                                                 float* __restrict__ gt_minmax) {
  __shared__ float s_mn[MINMAX_THREADS / 64], s_mx[MINMAX_THREADS / 64];
  const int b = blockIdx.x;
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const float* gb = gt + (long)b * HW;
  float mn = INFINITY, mx = -INFINITY;
  for (int i = threadIdx.x; i < HW; i += MINMAX_THREADS) {
    const float g = gb[i];
    mn = fminf(mn, g);
    mx = fmaxf(mx, g);
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    mn = fminf(mn, __shfl_xor(mn, o, 64));
    mx = fmaxf(mx, __shfl_xor(mx, o, 64));
  }
  if (lane == 0) {
    s_mn[w] = mn;
    s_mx[w] = mx;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    for (int i = 1; i < MINMAX_THREADS / 64; ++i) {
      mn = fminf(mn, s_mn[i]);
      mx = fmaxf(mx, s_mx[i]);
    }
    gt_minmax[2 * b] = mn;
    gt_minmax[2 * b + 1] = mx;
  }
}

// pure strategy: the first R_out candidates in draw order (no selection)
__global__ void copy_first_kernel(RankParams p) {
  const long per = (long)p.R_out * p.L * 2;
  const long total = (long)p.B * per;
  for (long e = (long)blockIdx.x * blockDim.x + threadIdx.x; e < total;
       e += (long)gridDim.x * blockDim.x) {
    const long b = e / per;
    const long r = e - b * per;
    p.out[e] = p.cand[b * (long)p.n_cand * p.L * 2 + r];
  }
}

static size_t align_up(size_t x) { return (x + 255) & ~(size_t)255; }

}  // namespace sampler_ex
}  // namespace pld

using namespace pld;
using namespace pld::sampler_ex;

static size_t rank_workspace(int B, int nc, int L) {
  return align_up(sizeof(float) * (size_t)B * nc * L * 2) + align_up(sizeof(double) * (size_t)B * nc);
}

// every launch of the rank step, arguments checked; p's own fields are filled by the caller
template <class Params>
static int rank_launch(const char* who, Params p, const float* gt, const int* valid_idx,
                       const int* nvalid, const float* gt_minmax, const int* draws, int B, int H,
                       int W, int R, int L, int nc, int strategy, float* out, void* ws,
                       void* stream) {
  const bool selects = strategy != PLD_SAMPLER_PURE;
  PLD_CHECK_ARG(!selects || sizeof(double) * (size_t)nc <= 150 * 1024,
                "%s: %d candidates exceed the LDS selection buffer", who, nc);
  p.gt = gt;
  p.valid_idx = valid_idx;
  p.nvalid = nvalid;
  p.gt_minmax = gt_minmax;
  p.draws = draws;
  p.B = B; p.H = H; p.W = W; p.L = L;
  p.n_cand = nc;
  p.strategy = strategy;
  p.R_out = std::min(nc, R);  // result_matrix[...][:batch_size]
  p.cand = (float*)ws;
  p.score = (double*)((char*)ws + align_up(sizeof(float) * (size_t)B * nc * L * 2));
  p.out = out;
  const RankParams& base = p;  // the selection kernels read the shared fields only
  hipStream_t st = as_stream(stream);
  const long total = (long)B * nc;
  const unsigned g = std::min<unsigned>(cdiv(total, 256), 8192);
  if (L <= 8) candidate_kernel<8, Params><<<g, 256, 0, st>>>(p);
  else if (L <= 64)
    candidate_wave_kernel<Params><<<std::min<unsigned>(cdiv(total, 4), 16384), 256, 0, st>>>(p);
  else candidate_kernel<512, Params><<<g, 256, 0, st>>>(p);
  int rc = check_launch("candidate_kernel");
  if (rc) return rc;
  if (!selects) {
    const long n = (long)B * p.R_out * L * 2;
    copy_first_kernel<<<std::min<unsigned>(cdiv(n, 256), 4096), 256, 0, st>>>(base);
    return check_launch("copy_first_kernel");
  }
  if (nc <= 1024) {
    select_kernel<<<B, 1024, sizeof(double) * nc, st>>>(base);
    return check_launch("select_kernel");
  }
  select_chunk_kernel<<<dim3(B, cdiv(nc, 256)), 256, sizeof(double) * nc, st>>>(base);
  return check_launch("select_chunk_kernel");
}

extern "C" int pld_sampler_rank_ex_workspace_size(int B, int n_cand, int L, size_t* bytes) {
  PLD_CHECK_ARG(bytes && B > 0 && n_cand > 0 && L > 0,
                "pld_sampler_rank_ex_workspace_size: bad args");
  *bytes = rank_workspace(B, n_cand, L);
  return PLD_OK;
}

extern "C" int pld_sampler_rank_ex(const float* gt, const int* valid_idx, const int* nvalid,
                                   const float* gt_minmax, const int* draws, int B, int H, int W,
                                   int mask_h, int mask_w, int R, int L, int n_cand, int strategy,
                                   double tau, double penalty, float* out, void* ws,
                                   size_t ws_bytes, void* stream) {
  PLD_CHECK_ARG(B > 0 && H > 0 && W > 0 && mask_h > 0 && mask_w > 0 && R > 0 && L > 0,
                "pld_sampler_rank_ex: bad args");
  PLD_CHECK_ARG(n_cand > 0, "pld_sampler_rank_ex: n_cand=%d must be positive", n_cand);
  PLD_CHECK_ARG(L <= 512, "pld_sampler_rank_ex: L=%d > 512", L);
  PLD_CHECK_ARG(strategy >= PLD_SAMPLER_PURE && strategy <= PLD_SAMPLER_RANDOM,
                "pld_sampler_rank_ex: bad strategy %d", strategy);
  PLD_CHECK_ARG(std::isfinite(tau) && tau >= 0.0,
                "pld_sampler_rank_ex: tau=%g must be finite and not negative", tau);
  PLD_CHECK_ARG(std::isfinite(penalty), "pld_sampler_rank_ex: penalty=%g must be finite", penalty);
  PLD_CHECK_ARG((long)H * W < (1 << 24) && (long)mask_h * mask_w < (1 << 24),
                "pld_sampler_rank_ex: H*W and mask_h*mask_w must stay below 2^24 (flat indices "
                "travel as float32)");
  PLD_CHECK_ARG(ws_bytes >= rank_workspace(B, n_cand, L),
                "pld_sampler_rank_ex: workspace of %zu bytes, %zu needed "
                "(pld_sampler_rank_ex_workspace_size)", ws_bytes, rank_workspace(B, n_cand, L));
  PLD_CHECK_ARG(strategy == PLD_SAMPLER_PURE || sizeof(double) * (size_t)n_cand <= 150 * 1024,
                "pld_sampler_rank_ex: %d candidates exceed the LDS selection buffer", n_cand);
  PLD_CHECK_ARG(gt && draws && out && ws, "pld_sampler_rank_ex: null pointer");
  if (strategy == PLD_SAMPLER_RANDOM)
    PLD_CHECK_ARG(!valid_idx && !nvalid, "pld_sampler_rank_ex: the unmasked strategy takes no "
                  "valid_idx / nvalid (a draw is the flat pixel)");
  else
    PLD_CHECK_ARG(valid_idx && nvalid, "pld_sampler_rank_ex: null valid_idx / nvalid");
  PLD_CHECK_ARG(valid_idx || (mask_h == H && mask_w == W),
                "pld_sampler_rank_ex: without valid_idx the mask grid is the image's");
  PLD_CHECK_ARG(strategy != PLD_SAMPLER_INFO || gt_minmax,
                "pld_sampler_rank_ex: Info needs gt_minmax");
  RankParamsEx p{};
  p.hi = (float)(1.0 + tau);
  p.lo = (float)(1.0 / (1.0 + tau));
  p.pen32 = (float)penalty;
  p.pen64 = penalty;
  p.mask_w = mask_w;
  p.mask_hw = mask_h * mask_w;
  p.scaled = mask_h != H || mask_w != W;
  p.xs = (double)H / (double)mask_h;
  p.ys = (double)W / (double)mask_w;
  return rank_launch("pld_sampler_rank_ex", p, gt, valid_idx, valid_idx ? nvalid : nullptr,
                     gt_minmax, draws, B, H, W, R, L, n_cand, strategy, out, ws, stream);
}

extern "C" int pld_sampler_minmax(const float* gt, int B, int H, int W, float* gt_minmax,
                                  void* stream) {
  PLD_CHECK_ARG(gt && gt_minmax && B > 0 && H > 0 && W > 0, "pld_sampler_minmax: bad args");
  PLD_CHECK_ARG((long)H * W < (1 << 24), "pld_sampler_minmax: H*W must stay below 2^24");
  minmax_kernel<<<B, MINMAX_THREADS, 0, as_stream(stream)>>>(gt, H * W, gt_minmax);
  return check_launch("minmax_kernel");
}

