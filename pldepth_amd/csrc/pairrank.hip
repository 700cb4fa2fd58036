// Pairwise ranking loss over the sampled lists, forward + closed-form backward:
// pld_pairrank_fwd_bwd, beside pld_listmle_fwd_bwd (listmle.hip) and
// pld_listmle_weighted_fwd_bwd (listmle_weighted.hip), which are left as they are.
//
// The loss the reference's method is compared with (Chen et al. 2016; Xian et al. 2018/2020),
// evaluated on the lists the samplers emit, with the reference's own depth relation
// (pldepth/data/depth_utils.py:5-36) at the threshold its --equality_threshold carries and its
// pair tables keep z0, z1 for (generic_ranking_provider.py:108). With t_i = pred[b, idx_i], for
// every valid pair (i, j), i before j in list order ("all": every i < j; "adjacent": j = i + 1),
// r = relation(z_i, z_j) (negated by `invert`), d = t_i - t_j:
//   r != 0: l = softplus(-r d) = max(-r d, 0) + log1p(exp(-|d|)),  dl/dt_i = -r sigmoid(-r d)
//   r == 0: l = equal_weight d^2,                                  dl/dt_i = 2 equal_weight d
//   dl/dt_j = -dl/dt_i
//   loss_n = sum l / n_n (n_n valid pairs; 0 pairs: 0),  per_list[n] = s_n loss_n
//   loss = sum_n s_n loss_n (/ N for the mean)
// An element is valid when its label is >= 0 (pld_listmle_fwd_bwd's rule); a pair when both are.
//
// One wave64 per list, four lists per 256-thread block. Lane l owns elements l, l + 64, ...
// (EPL = ceil(L / 64) of them): the list's gathered logits and depths are staged in LDS, and
// each lane walks the partners of its own elements by their cyclic distance `off`, element e
// meeting (e + off) mod L, so that the lanes of a wave read consecutive LDS words and whether a
// distance carries the pair's loss term is the same for the whole wave: every unordered pair is
// met twice, once from each end (each end needs the pair's gradient; a list does no atomics
// among its own elements), and the end that meets it at the shorter distance adds its loss
// term, so log1p is evaluated on the first half of the distances only. "all" costs
// EPL (L - 1) pair evaluations per lane (8 x 511 at L = 512), "adjacent" two per element.
// Element gradients accumulate in fp32 registers, the list's loss in fp64 (130,816 positive
// terms at L = 512); s_n, 1 / n_n and 1 / N are applied as one factor at the end, and each valid
// element issues one atomicAdd into dpred, as ListMLE's scatter does.
#include <algorithm>
#include <cmath>

#include "common.h"

namespace pld {
namespace pairrank {

constexpr long PR_MAX_PIXELS = 1L << 24;  // flat indices are stored as float32

struct Rel {
  float hi, lo;  // float32(1 + tau), float32(1 / (1 + tau)), formed in double by the host
  int plain;     // tau < 0 (threshold=None): z_i > z_j, z_i < z_j
  int invert;
};

__device__ __forceinline__ int relation(float zi, float zj, Rel t) {
  const int r = t.plain ? (zi > zj) - (zi < zj) : depth_relation32(zi, zj, t.hi, t.lo);
  return t.invert ? -r : r;
}

// One pair, i before j in list order: dl/dt_i (= -dl/dt_j), and the loss term when LOSS.
// One exp serves the softplus and the sigmoid: with e = exp(-|d|), sigmoid(x) is 1 / (1 + e)
// for x >= 0 and e / (1 + e) below.
template <bool LOSS>
__device__ __forceinline__ float pair_term(float ti, float tj, float zi, float zj, Rel rel,
                                           float ew, float& l) {
  const int r = relation(zi, zj, rel);
  const float d = ti - tj;
  if (r == 0) {
    const float wd = ew * d;
    if (LOSS) l = wd * d;
    return 2.f * wd;
  }
  const float x = r > 0 ? -d : d;  // -r d
  const float e = expf(-fabsf(d));
  const float inv = __builtin_amdgcn_rcpf(1.f + e);
  const float sig = x >= 0.f ? inv : e * inv;
  if (LOSS) l = fmaxf(x, 0.f) + log1pf(e);
  return r > 0 ? -sig : sig;
}

template <int EPL>
__global__ __launch_bounds__(256) void pair_kernel(
    const float* __restrict__ pred, const float* __restrict__ y_true, int B, int HW, int R, int L,
    int adjacent, Rel rel, float ew, const float* __restrict__ list_w, int list_w_per_image,
    double red_scale, float* __restrict__ per_list, float* __restrict__ dpred) {
  constexpr int WAVES = 4;
  constexpr int LMAX = 64 * EPL;
  __shared__ float s_t[WAVES][LMAX];
  __shared__ float s_z[WAVES][LMAX];
  const int wave = threadIdx.x >> 6;
  const int lane = threadIdx.x & 63;
  const long list = (long)blockIdx.x * WAVES + wave;
  const bool active = list < (long)B * R;  // wave-uniform; inactive waves still reach the barrier
  const int b = active ? (int)(list / R) : 0;
  if (!active) L = 0;
  const float* yt = y_true + (active ? list : 0) * (long)L * 2;
  const float* pb = pred + (long)b * HW;

  float t[EPL], z[EPL], g[EPL];
  int idx[EPL];
  bool ok[EPL];  // in the list and valid
#pragma unroll
  for (int q = 0; q < EPL; ++q) {
    const int e = q * 64 + lane;
    t[q] = 0.f;
    z[q] = -1.f;
    g[q] = 0.f;
    idx[q] = -1;
    ok[q] = false;
    if (e < L) {
      const float fi = yt[2 * e];
      const float lab = yt[2 * e + 1];
      const int ii = (int)fi;  // tf.cast(float32 -> int32): truncation
      idx[q] = ii;
      t[q] = (ii >= 0 && ii < HW) ? pb[ii] : 0.f;  // TF GPU gather yields 0 out of range
      ok[q] = lab >= 0.f;
      z[q] = ok[q] ? lab : -1.f;  // a NaN label is invalid too
      s_t[wave][e] = t[q];
      s_z[wave][e] = z[q];
    }
  }
  __syncthreads();  // s_t and s_z are staged; each wave reads its own rows only
  if (!active) return;

  double lsum = 0.0;
  int cnt = 0;
  if (adjacent) {
#pragma unroll
    for (int q = 0; q < EPL; ++q) {
      const int e = q * 64 + lane;
      if (!ok[q]) continue;
      if (e + 1 < L && s_z[wave][e + 1] >= 0.f) {  // (e, e + 1): this end adds the loss term
        float l = 0.f;
        g[q] += pair_term<true>(t[q], s_t[wave][e + 1], z[q], s_z[wave][e + 1], rel, ew, l);
        lsum += (double)l;
        ++cnt;
      }
      if (e >= 1 && s_z[wave][e - 1] >= 0.f) {  // (e - 1, e)
        float l;
        g[q] -= pair_term<false>(s_t[wave][e - 1], t[q], s_z[wave][e - 1], z[q], rel, ew, l);
      }
    }
  } else {
    // distances 1 .. L/2 carry the loss term (at 2 off == L both ends meet the pair at the same
    // distance: the end that does not wrap adds it), distances above only the gradient
    const int half = L >> 1;
    for (int off = 1; off <= half; ++off) {
      const bool both = 2 * off == L;
#pragma unroll
      for (int q = 0; q < EPL; ++q) {
        int j = q * 64 + lane + off;
        const bool wrap = j >= L;
        if (wrap) j -= L;
        if (!ok[q]) continue;
        const float tj = s_t[wave][j], zj = s_z[wave][j];
        if (!(zj >= 0.f)) continue;
        float l = 0.f;
        const float gi = pair_term<true>(wrap ? tj : t[q], wrap ? t[q] : tj, wrap ? zj : z[q],
                                         wrap ? z[q] : zj, rel, ew, l);
        g[q] += wrap ? -gi : gi;
        if (!(both && wrap)) {
          lsum += (double)l;
          ++cnt;
        }
      }
    }
    for (int off = half + 1; off < L; ++off) {
#pragma unroll
      for (int q = 0; q < EPL; ++q) {
        int j = q * 64 + lane + off;
        const bool wrap = j >= L;
        if (wrap) j -= L;
        if (!ok[q]) continue;
        const float tj = s_t[wave][j], zj = s_z[wave][j];
        if (!(zj >= 0.f)) continue;
        float l;
        const float gi = pair_term<false>(wrap ? tj : t[q], wrap ? t[q] : tj, wrap ? zj : z[q],
                                          wrap ? z[q] : zj, rel, ew, l);
        g[q] += wrap ? -gi : gi;
      }
    }
  }
  lsum = wave_sum(lsum);
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) cnt += __shfl_xor(cnt, o, 64);

  float sw = 1.f;  // the list's sample weight
  if (list_w) sw = list_w[list_w_per_image ? (long)b : list];
  // s_n / n_n (x 1/N for the mean) as one factor: a power-of-two s_n scales everything exactly
  const double per_pair = cnt > 0 ? (double)sw / (double)cnt : 0.0;
  const float gscale = (float)(per_pair * red_scale);
#pragma unroll
  for (int q = 0; q < EPL; ++q) {
    if (ok[q] && idx[q] >= 0 && idx[q] < HW)
      atomicAdd(dpred + (long)b * HW + idx[q], g[q] * gscale);
  }
  if (lane == 0) per_list[list] = cnt > 0 ? (float)(lsum * per_pair) : 0.f;
}

// deterministic sum (or mean) of the weighted per-list losses (single block, fp64 accumulation,
// fixed order: the loss value is the same from replay to replay)
__global__ __launch_bounds__(256) void reduce_kernel(const float* __restrict__ x, long n,
                                                     int mean, float* __restrict__ out) {
  __shared__ double red[256];
  double acc = 0.0;
  for (long i = threadIdx.x; i < n; i += 256) acc += (double)x[i];
  red[threadIdx.x] = acc;
  __syncthreads();
  for (int s = 128; s > 0; s >>= 1) {
    if ((int)threadIdx.x < s) red[threadIdx.x] += red[threadIdx.x + s];
    __syncthreads();
  }
  if (threadIdx.x == 0) out[0] = (float)(mean ? red[0] / (double)n : red[0]);
}

// dpred = 0 ahead of the scatter: a kernel, not a memset node, for the reason given at
// listmle.hip's zero_kernel (a captured memset was not ordered before the scatter on replay)
__global__ __launch_bounds__(256) void zero_kernel(float* __restrict__ p, long n) {
  const long n4 = n >> 2;
  const long stride = (long)gridDim.x * blockDim.x;
  float4* p4 = reinterpret_cast<float4*>(p);
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += stride)
    p4[i] = make_float4(0.f, 0.f, 0.f, 0.f);
  for (long i = 4 * n4 + (long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride)
    p[i] = 0.f;
}

}  // namespace pairrank
}  // namespace pld

extern "C" int pld_pairrank_fwd_bwd(const float* pred, const float* y_true, int B, int HW, int R,
                                    int L, int pair_mode, double tau, int invert,
                                    float equal_weight, const float* list_w, int list_w_per_image,
                                    int reduction, float* per_list, float* loss, float* dpred,
                                    int zero_dpred, void* stream) {
  using namespace pld;
  using namespace pld::pairrank;
  // every scalar first: nothing below looks at a pointer or launches before these pass
  PLD_CHECK_ARG(B > 0 && HW > 0 && R > 0 && L >= 2 && L <= 512,
                "pld_pairrank_fwd_bwd: bad shape B=%d HW=%d R=%d L=%d (L must be 2..512)", B, HW,
                R, L);
  PLD_CHECK_ARG((long)HW <= PR_MAX_PIXELS,
                "pld_pairrank_fwd_bwd: HW=%d pixels: flat indices are float32 (limit 2^24)", HW);
  PLD_CHECK_ARG(pair_mode == PLD_PAIRS_ALL || pair_mode == PLD_PAIRS_ADJACENT,
                "pld_pairrank_fwd_bwd: unknown pair_mode %d", pair_mode);
  PLD_CHECK_ARG(reduction == PLD_REDUCE_MEAN || reduction == PLD_REDUCE_SUM,
                "pld_pairrank_fwd_bwd: unknown reduction %d", reduction);
  PLD_CHECK_ARG(std::isfinite(tau), "pld_pairrank_fwd_bwd: tau must be finite (negative: the "
                "plain comparison)");
  PLD_CHECK_ARG(std::isfinite(equal_weight) && equal_weight >= 0.f,
                "pld_pairrank_fwd_bwd: equal_weight must be finite and >= 0");
  PLD_CHECK_ARG(pred && y_true && per_list && loss && dpred,
                "pld_pairrank_fwd_bwd: null pointer");
  PLD_CHECK_ARG(!zero_dpred || aligned16(dpred), "pld_pairrank_fwd_bwd: dpred must be "
                "16-byte aligned");
  hipStream_t st = as_stream(stream);
  if (zero_dpred) {
    const long nz = (long)B * HW;
    pairrank::zero_kernel<<<(unsigned)std::min<long>(cdiv(nz / 4 + 1, 256), 4096), 256, 0, st>>>(
        dpred, nz);
    int rc = check_launch("pairrank::zero_kernel");
    if (rc) return rc;
  }
  Rel rel;
  rel.plain = tau < 0.0;
  rel.hi = (float)(1.0 + (rel.plain ? 0.0 : tau));
  rel.lo = (float)(1.0 / (1.0 + (rel.plain ? 0.0 : tau)));
  rel.invert = invert != 0;
  const long n = (long)B * R;
  const int mean = reduction == PLD_REDUCE_MEAN;
  const double red_scale = mean ? 1.0 / (double)n : 1.0;
  const int adjacent = pair_mode == PLD_PAIRS_ADJACENT;
  const int per_image = list_w_per_image != 0;
  dim3 grid(cdiv(n, 4)), block(256);
  if (L <= 64)
    pair_kernel<1><<<grid, block, 0, st>>>(pred, y_true, B, HW, R, L, adjacent, rel,
                                           equal_weight, list_w, per_image, red_scale, per_list,
                                           dpred);
  else if (L <= 128)
    pair_kernel<2><<<grid, block, 0, st>>>(pred, y_true, B, HW, R, L, adjacent, rel,
                                           equal_weight, list_w, per_image, red_scale, per_list,
                                           dpred);
  else if (L <= 256)
    pair_kernel<4><<<grid, block, 0, st>>>(pred, y_true, B, HW, R, L, adjacent, rel,
                                           equal_weight, list_w, per_image, red_scale, per_list,
                                           dpred);
  else
    pair_kernel<8><<<grid, block, 0, st>>>(pred, y_true, B, HW, R, L, adjacent, rel,
                                           equal_weight, list_w, per_image, red_scale, per_list,
                                           dpred);
  int rc = check_launch("pairrank::pair_kernel");
  if (rc) return rc;
  pairrank::reduce_kernel<<<1, 256, 0, st>>>(per_list, n, mean, loss);
  return check_launch("pairrank::reduce_kernel");
}
