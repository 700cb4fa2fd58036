// Position-weighted ListMLE (p-ListMLE) forward + closed-form backward with per-list sample
// weights and a choice of reduction: pld_listmle_weighted_fwd_bwd, beside pld_listmle_fwd_bwd
// (listmle.hip), which is left as it is.
//
// Replaces what the reference forwards into tensorflow_ranking when a lambda weight is given
// (pldepth/losses/nll_loss.py:11-16, 33-40: ListMLELoss(lambda_weight=ListMLELambdaWeight(f))),
// Keras' compute_weighted_loss (sample_weight) and its SUM / SUM_OVER_BATCH_SIZE reductions:
//   w_r   = f(float32(r)), r = 1..L in sorted order (ListMLELambdaWeight.individual_weights)
//   nll   = sum_r w_r (log C_r - (t_r - m)),      C_r = sum_{j>=r} exp(t_j - m), m = max t
//   d nll / d t_k = exp(t_k - m) sum_{r<=k} w_r / C_r - w_k
//   nll_out[n] = s_n nll_n;  loss = sum_n s_n nll_n (/ N for the mean)
// Everything up to the sorted, max-shifted logits (gather, validity, sort by label, tie order) is
// listmle_kernel's, statement for statement: this is a second copy rather than a template flag
// on that kernel so that its instances, which every unweighted step runs, compile exactly as
// before (instances of one template share their register allocation context).
//
// One wave64 per list, EPL consecutive elements per lane. The L rank weights are the same for
// every list: the block's 256 threads stage them in LDS with one coalesced read (thread i reads
// rank_w[i]), and each lane then takes its EPL consecutive ranks from there.
#include <algorithm>

#include "common.h"

namespace pld {
namespace listmle_w {

constexpr float kLogEps = -23.025850929940457f;  // tf.math.log(1e-10) in float32

template <int EPL>
__global__ __launch_bounds__(256) void weighted_kernel(
    const float* __restrict__ pred, const float* __restrict__ y_true, int B, int HW, int R, int L,
    const float* __restrict__ rank_w, const float* __restrict__ list_w, int list_w_per_image,
    float red_scale, float* __restrict__ nll_out, float* __restrict__ dpred) {
  constexpr int WAVES = 4;
  constexpr int LMAX = 64 * EPL;
  __shared__ float s_key[WAVES][LMAX];
  __shared__ float s_val[WAVES][LMAX];
  __shared__ float s_w[LMAX];
  const int wave = threadIdx.x >> 6;
  const int lane = threadIdx.x & 63;
  const long list = (long)blockIdx.x * WAVES + wave;
  const long nlists = (long)B * R;
  const bool active = list < nlists;  // wave-uniform; inactive waves still reach the barriers
  const int b = active ? (int)(list / R) : 0;
  // rank weights, staged by the whole block (inactive waves included: L is still the caller's)
  for (int i = threadIdx.x; i < L; i += 256) s_w[i] = rank_w ? rank_w[i] : 1.f;
  if (!active) L = 0;
  const float* yt = y_true + (active ? list : 0) * (long)L * 2;
  const float* pb = pred + (long)b * HW;
  float sw = 1.f;  // the list's sample weight
  if (active && list_w) sw = list_w[list_w_per_image ? (long)b : list];

  float s[EPL], lab[EPL];
  int idx[EPL];
  bool valid[EPL], inl[EPL];
  float minlab = INFINITY;
#pragma unroll
  for (int q = 0; q < EPL; ++q) {
    const int e = lane * EPL + q;
    inl[q] = e < L;
    idx[q] = -1;
    s[q] = 0.f;
    lab[q] = 0.f;
    valid[q] = false;
    if (inl[q]) {
      const float fi = yt[2 * e];
      lab[q] = yt[2 * e + 1];
      const int ii = (int)fi;  // tf.cast(float32 -> int32): truncation
      idx[q] = ii;
      s[q] = (ii >= 0 && ii < HW) ? pb[ii] : 0.f;  // TF GPU gather yields 0 out of range
      valid[q] = lab[q] >= 0.f;
      if (!valid[q]) lab[q] = 0.f;
      minlab = fminf(minlab, lab[q]);
    }
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) minlab = fminf(minlab, __shfl_xor(minlab, o, 64));
  // sort scores: valid -> label, invalid -> min(label') - 1e-6 (float32)
#pragma unroll
  for (int q = 0; q < EPL; ++q) {
    const int e = lane * EPL + q;
    if (inl[q]) s_key[wave][e] = valid[q] ? lab[q] : (minlab - 1e-6f);
    if (!valid[q]) s[q] = kLogEps;
  }
  __syncthreads();  // s_key and s_w are staged
  int rank[EPL];
#pragma unroll
  for (int q = 0; q < EPL; ++q) {
    const int e = lane * EPL + q;
    int r = 0;
    if (inl[q]) {
      const float k = s_key[wave][e];
      for (int j = 0; j < L; ++j) {
        const float kj = s_key[wave][j];
        r += (kj > k) | ((kj == k) & (j > e));
      }
    }
    rank[q] = r;
  }
#pragma unroll
  for (int q = 0; q < EPL; ++q)
    if (inl[q]) s_val[wave][rank[q]] = s[q];
  __syncthreads();
  // sorted logits t_r and their rank weights w_r, r = lane*EPL + q (rank r + 1 of tfr's 1..L)
  float t[EPL], w[EPL];
  float m = -INFINITY;
#pragma unroll
  for (int q = 0; q < EPL; ++q) {
    const int r = lane * EPL + q;
    t[q] = (r < L) ? s_val[wave][r] : -INFINITY;
    w[q] = (r < L) ? s_w[r] : 0.f;
    m = fmaxf(m, t[q]);
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) m = fmaxf(m, __shfl_xor(m, o, 64));
  float ex[EPL];
  float lsum = 0.f;
#pragma unroll
  for (int q = 0; q < EPL; ++q) {
    const int r = lane * EPL + q;
    ex[q] = (r < L) ? expf(t[q] - m) : 0.f;
    lsum += ex[q];
  }
  // suffix (reverse inclusive) sum over ranks: C_r = sum_{j>=r} ex_j
  // lanes above contribute their whole chunk sums: exclusive suffix scan across lanes
  // (exclusive scans are formed by shifting first, never by subtracting: the last ranks can
  // carry w/C ~ 1e10 when invalid elements sit there, and a difference would cancel)
  float above = __shfl_down(lsum, 1, 64);
  if (lane == 63) above = 0.f;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const float v = __shfl_down(above, o, 64);
    if (lane + o < 64) above += v;
  }  // sum of the chunks of lanes > lane
  float C[EPL];
  {
    float run = above;
#pragma unroll
    for (int q = EPL - 1; q >= 0; --q) {
      run += ex[q];
      C[q] = run;
    }
  }
  float part = 0.f, pinv = 0.f;
  float winv[EPL];
#pragma unroll
  for (int q = 0; q < EPL; ++q) {
    const int r = lane * EPL + q;
    if (r < L) {
      part += w[q] * (logf(C[q]) - (t[q] - m));
      winv[q] = w[q] / C[q];
    } else {
      winv[q] = 0.f;
    }
    pinv += winv[q];
  }
  const float nll = wave_sum(part);
  // prefix (inclusive) sum of w/C over ranks
  float run = __shfl_up(pinv, 1, 64);
  if (lane == 0) run = 0.f;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const float v = __shfl_up(run, o, 64);
    if (lane >= o) run += v;
  }  // sum of the chunks of lanes < lane
  __syncthreads();
#pragma unroll
  for (int q = 0; q < EPL; ++q) {
    const int r = lane * EPL + q;
    run += winv[q];
    if (r < L) s_val[wave][r] = ex[q] * run - w[q];  // d nll / d t_r
  }
  __syncthreads();
  // s_n (x 1/N for the mean): a power-of-two s_n scales every gradient exactly
  const float gscale = sw * red_scale;
#pragma unroll
  for (int q = 0; q < EPL; ++q) {
    if (inl[q] && valid[q] && idx[q] >= 0 && idx[q] < HW) {
      const float g = s_val[wave][rank[q]] * gscale;
      atomicAdd(dpred + (long)b * HW + idx[q], g);
    }
  }
  if (active && lane == 0) nll_out[list] = sw * nll;
}

// deterministic sum (or mean) of the weighted per-list nll (single block, fp64 accumulation)
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

}  // namespace listmle_w
}  // namespace pld

extern "C" int pld_listmle_weighted_fwd_bwd(const float* pred, const float* y_true, int B, int HW,
                                            int R, int L, const float* rank_w,
                                            const float* list_w, int list_w_per_image,
                                            int reduction, float* nll, float* loss, float* dpred,
                                            int zero_dpred, void* stream) {
  using namespace pld;
  using namespace pld::listmle_w;
  PLD_CHECK_ARG(pred && y_true && nll && loss && dpred,
                "pld_listmle_weighted_fwd_bwd: null pointer");
  PLD_CHECK_ARG(B > 0 && HW > 0 && R > 0 && L >= 1 && L <= 512,
                "pld_listmle_weighted_fwd_bwd: bad shape B=%d HW=%d R=%d L=%d (L must be 1..512)",
                B, HW, R, L);
  PLD_CHECK_ARG(reduction == PLD_REDUCE_MEAN || reduction == PLD_REDUCE_SUM,
                "pld_listmle_weighted_fwd_bwd: unknown reduction %d", reduction);
  hipStream_t st = as_stream(stream);
  PLD_CHECK_ARG(!zero_dpred || aligned16(dpred), "pld_listmle_weighted_fwd_bwd: dpred must be "
                "16-byte aligned");
  if (zero_dpred) {
    const long nz = (long)B * HW;
    listmle_w::zero_kernel<<<(unsigned)std::min<long>(cdiv(nz / 4 + 1, 256), 4096), 256, 0,
                             st>>>(dpred, nz);
    int rc = check_launch("listmle_w::zero_kernel");
    if (rc) return rc;
  }
  const long n = (long)B * R;
  const int mean = reduction == PLD_REDUCE_MEAN;
  const float red_scale = mean ? (float)(1.0 / (double)n) : 1.f;
  const int per_image = list_w_per_image != 0;
  dim3 grid(cdiv(n, 4)), block(256);
  if (L <= 64)
    weighted_kernel<1><<<grid, block, 0, st>>>(pred, y_true, B, HW, R, L, rank_w, list_w,
                                               per_image, red_scale, nll, dpred);
  else if (L <= 128)
    weighted_kernel<2><<<grid, block, 0, st>>>(pred, y_true, B, HW, R, L, rank_w, list_w,
                                               per_image, red_scale, nll, dpred);
  else if (L <= 256)
    weighted_kernel<4><<<grid, block, 0, st>>>(pred, y_true, B, HW, R, L, rank_w, list_w,
                                               per_image, red_scale, nll, dpred);
  else
    weighted_kernel<8><<<grid, block, 0, st>>>(pred, y_true, B, HW, R, L, rank_w, list_w,
                                               per_image, red_scale, nll, dpred);
  int rc = check_launch("listmle_w::weighted_kernel");
  if (rc) return rc;
  listmle_w::reduce_kernel<<<1, 256, 0, st>>>(nll, n, mean, loss);
  return check_launch("listmle_w::reduce_kernel");
}
