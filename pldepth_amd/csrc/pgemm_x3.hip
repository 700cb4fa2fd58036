// Deep-K, narrow-N 1x1 convolutions on bf16x3 MFMA whose input operand is produced on the fly by
// the elementwise op that precedes them (pgemm.hip's two prologues, for the MBConv blocks whose
// filter no longer fits pgemm.hip's scalar-cache FMA scheme):
//   PRO_BNACT : y[m][n] = sum_k (act(bn(x[m][k])) * gate[img(m)][k]) * w[n][k]
//               — blocks 3a..7a project conv (K = cexp = 144..1152, N = cout = 40..320) reading
//                 dw_pre; replaces pld_bn_apply(gate) + pld_conv2d_fwd, se_excite is not written;
//   PRO_BNBWD : y[m][n] (+)= sum_k bnbwd(x, dy)[m][k] * w[n][k]
//               — blocks 3b..7a expand dgrad (K = cexp = 240..1152, N = cin = 40..192) reading
//                 (expand_pre, d expand_activation) and k12 from pld_bn_bwd_coeffs; replaces the
//                 apply pass of pld_bn_bwd + pld_conv2d_dgrad, the pre-BN gradient is not written.
// The staged operand is bit for bit what bn_apply_kernel / bn_bwd_apply_kernel would have written
// (their operation order with every rounding pinned); the product is the project's bf16x3: hi = bf16(v),
// lo = bf16(v - hi), lo*hi + hi*lo + hi*hi per 16-k step on v_mfma_f32_32x32x16_bf16, fp32
// accumulation, K ascending. The filter is the pld_filter_split copy.
//
// A workgroup owns BM = 32 or 64 consecutive rows and ALL N columns (N <= 320), so the operand is
// read once. K streams through LDS in chunks of 64 as hi/lo bf16 planes, two buffers, one barrier
// per chunk, warp-specialised as wide1x1.hip (gfx950 counts loads and stores in one vmcnt):
//   4 loader waves : 16-byte loads of chunk i+2 / i+3 in two register stages; chunk i+1 goes
//                    through the prologue (two quarter-rate transcendentals per element for
//                    swish: hence four waves) and the hi/lo split into LDS. The BN vectors sit
//                    in LDS for the whole launch and are read per chunk, not held in registers.
//   4 compute waves: A fragments from LDS, filter fragments straight from the split copy in L2
//                    (one 16-k step ahead; every workgroup reads the whole filter, <= 1.4 MB, so
//                    it stays in each XCD's L2 whatever the workgroup order), 3 MFMAs per
//                    32x32 tile and step; the output tile leaves through LDS as float4 row
//                    segments once the K loop is done.
// No atomics, no workspace, no memset: graph-safe and deterministic.
#include <algorithm>

#include "common.h"
#include "conv_common.h"

namespace pld {
namespace px3 {

typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef unsigned int u32x2 __attribute__((ext_vector_type(2)));
typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));

enum Pro { PRO_BNACT = 0, PRO_BNBWD = 1 };

struct Params {
  const float* x;       // [M][K]
  const float* dy;      // [M][K] (PRO_BNBWD)
  const float* mean;
  const float* invstd;
  const float* gamma;
  const float* beta;
  const float* gate;    // [n_img][K] or NULL (PRO_BNACT)
  const float* k12;     // [2][K] (PRO_BNBWD)
  const u32x4* ws;      // [N][K / 8] chunks of {8 bf16 hi, 8 bf16 lo} (pld_filter_split)
  float* y;             // [M][N]
  int M, K, N, act, acc;
  FastDiv dHW;          // rows per image (gate)
};

constexpr int KC = 64;            // k per LDS chunk: four 16-k MFMA steps
constexpr int RS = 2 * KC + 16;   // row pitch in bytes of one plane: an odd multiple of 16
constexpr int NCW = 4, NLW = 4;   // compute / loader waves
constexpr int OLS = 40;           // row pitch (floats) of a compute wave's output staging tile
constexpr int OBUF_BYTES = NCW * 32 * OLS * 4;
constexpr int K_MAX = 1152, N_MAX = 320;

// 4 floats -> packed bf16 hi / lo quads (wide1x1.hip's split4; through scalars: a bit_cast of a
// vector-element lvalue reads element 0 on this ROCm)
__device__ __forceinline__ void split4(const float (&f)[4], u32x2& hi, u32x2& lo) {
  unsigned short hs[4], ls[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const __bf16 h = (__bf16)f[i];
    // add_rn: the residual of the ROUNDED value (left to the compiler, the product that formed
    // f[i] fused into this subtraction and lo came from the unrounded one)
    const __bf16 l = (__bf16)add_rn(f[i], -(float)h);
    hs[i] = __builtin_bit_cast(unsigned short, h);
    ls[i] = __builtin_bit_cast(unsigned short, l);
  }
  hi = u32x2{hs[0] | (unsigned)hs[1] << 16, hs[2] | (unsigned)hs[3] << 16};
  lo = u32x2{ls[0] | (unsigned)ls[1] << 16, ls[2] | (unsigned)ls[3] << 16};
}

// LDS hand-off (wide1x1.hip): the ds operations complete, the loaders' prefetches stay in flight
__device__ __forceinline__ void lds_barrier() {
  asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
  __builtin_amdgcn_s_barrier();
  asm volatile("" ::: "memory");
}

template <int TM, int WR>
constexpr int a_region_bytes() {
  return std::max(2 * 2 * (32 * TM * WR) * RS, OBUF_BYTES);
}

// TM: 32-row tiles per compute wave; WR: compute waves along the rows (NCW / WR along the
// columns); TN: 32-column tiles per compute wave. BM = 32 TM WR rows per workgroup.
template <int PRO, int TM, int WR, int TN>
__global__ __launch_bounds__((NCW + NLW) * 64) void pgemm_x3_kernel(Params p) {
  constexpr int BM = 32 * TM * WR, P = BM / 16;
  constexpr int PLANE = BM * RS, BUF = 2 * PLANE;
  constexpr int NV = PRO == PRO_BNBWD ? 6 : 4;
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  float* prm = reinterpret_cast<float*>(smem + a_region_bytes<TM, WR>());  // [NV][K]
  const int K = p.K, M = p.M, N = p.N;
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const long m0 = (long)blockIdx.x * BM;
  const int nch = (K + KC - 1) / KC;

  // the BN vectors (and k1, k2) of all K channels: LDS for the whole launch
  for (int e = threadIdx.x; e < K / 4; e += (NCW + NLW) * 64) {
    float4* d = reinterpret_cast<float4*>(prm) + e;
    const int kq = K / 4;
    d[0] = reinterpret_cast<const float4*>(p.mean)[e];
    d[kq] = reinterpret_cast<const float4*>(p.invstd)[e];
    d[2 * kq] = reinterpret_cast<const float4*>(p.gamma)[e];
    d[3 * kq] = reinterpret_cast<const float4*>(p.beta)[e];
    if (PRO == PRO_BNBWD) {
      d[4 * kq] = reinterpret_cast<const float4*>(p.k12)[e];
      d[5 * kq] = reinterpret_cast<const float4*>(p.k12 + K)[e];
    }
  }
  __syncthreads();

  if (wave >= NCW) {
    // ---- loader waves. Thread (r0 = lt / 16, q = lt % 16) owns the 4-k quad q of rows r0,
    // r0 + 16, ... of every chunk: one channel quad per chunk, its BN vectors read once per
    // chunk. Rows past M and quads past K are clamped (their products are never read / stored).
    const int lt = threadIdx.x - NCW * 64;
    const int q = lt & 15, r0 = lt >> 4;
    struct Stage {
      float4 a[P], b[P];
    };
    auto load = [&](int ch, Stage& s) {
      const int c = min(ch * KC + 4 * q, K - 4);
#pragma unroll
      for (int j = 0; j < P; ++j) {
        const long row = min(m0 + r0 + 16 * j, (long)M - 1);
        s.a[j] = *reinterpret_cast<const float4*>(p.x + row * K + c);
        if (PRO == PRO_BNBWD) {
          s.b[j] = *reinterpret_cast<const float4*>(p.dy + row * K + c);
        } else if (p.gate) {
          const long img = (long)p.dHW.div((uint32_t)row);
          s.b[j] = *reinterpret_cast<const float4*>(p.gate + img * K + c);
        } else {
          s.b[j] = make_float4(1.f, 1.f, 1.f, 1.f);
        }
      }
    };
    auto store = [&](int ch, const Stage& s) {
      unsigned char* hi = smem + (ch & 1) * BUF;
      const int c = min(ch * KC + 4 * q, K - 4);
      const float4 mu4 = *reinterpret_cast<const float4*>(prm + c);
      const float4 is4 = *reinterpret_cast<const float4*>(prm + K + c);
      const float4 ga4 = *reinterpret_cast<const float4*>(prm + 2 * K + c);
      const float4 be4 = *reinterpret_cast<const float4*>(prm + 3 * K + c);
      const float mu[4] = {mu4.x, mu4.y, mu4.z, mu4.w}, is[4] = {is4.x, is4.y, is4.z, is4.w};
      const float ga[4] = {ga4.x, ga4.y, ga4.z, ga4.w}, be[4] = {be4.x, be4.y, be4.z, be4.w};
      float k1[4] = {0.f, 0.f, 0.f, 0.f}, k2[4] = {0.f, 0.f, 0.f, 0.f};
      if (PRO == PRO_BNBWD) {
        const float4 k14 = *reinterpret_cast<const float4*>(prm + 4 * K + c);
        const float4 k24 = *reinterpret_cast<const float4*>(prm + 5 * K + c);
        k1[0] = k14.x; k1[1] = k14.y; k1[2] = k14.z; k1[3] = k14.w;
        k2[0] = k24.x; k2[1] = k24.y; k2[2] = k24.z; k2[3] = k24.w;
      }
#pragma unroll
      for (int j = 0; j < P; ++j) {
        const float xs[4] = {s.a[j].x, s.a[j].y, s.a[j].z, s.a[j].w};
        const float bs[4] = {s.b[j].x, s.b[j].y, s.b[j].z, s.b[j].w};
        float o[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
          // The roundings are pinned (fmaf / mul_rn / add_rn) to the instruction sequence the BN
          // kernels compile to: one fma for xh ga + be and for the - xh k2 term, every other
          // product and sum rounded on its own. Left to -ffp-contract=fast the compiler fused
          // the last product into the hi/lo split and left single elements of a quad unfused.
          const float xh = (xs[u] - mu[u]) * is[u];
          const float z = fmaf(xh, ga[u], be[u]);
          if (PRO == PRO_BNACT) {  // bn_apply_kernel: bn, then act, then the gate
            o[u] = mul_rn(act_fwd(p.act, z), bs[u]);
          } else {  // bn_bwd_apply_kernel (bn_bwd_dz / bn_bwd_dx with gate 1, no squeeze term,
                    // no residual)
            float ag;
            if (p.act == ACT_SWISH) {
              const float sg = sigmoidf_(z);
              ag = mul_rn(sg, fmaf(z, add_rn(1.f, -sg), 1.f));
            } else {
              ag = act_grad(p.act, z);
            }
            const float dz = mul_rn(add_rn(bs[u], 0.f), ag);
            const float t = fmaf(-xh, k2[u], add_rn(dz, -k1[u]));
            o[u] = mul_rn(mul_rn(is[u], ga[u]), t);
          }
        }
        u32x2 h, l;
        split4(o, h, l);
        const int off = (r0 + 16 * j) * RS + 8 * q;
        *reinterpret_cast<u32x2*>(hi + off) = h;
        *reinterpret_cast<u32x2*>(hi + PLANE + off) = l;
      }
    };
    // chunk j goes to LDS buffer j & 1; two register stages; barriers: 1 + nch (the compute
    // waves' count)
    Stage s0, s1;
    load(0, s0);
    store(0, s0);
    if (nch > 1) load(1, s0);
    if (nch > 2) load(2, s1);
    lds_barrier();
    for (int i = 0;; i += 2) {
      if (i + 1 < nch) store(i + 1, s0);
      if (i + 3 < nch) load(i + 3, s0);
      lds_barrier();
      if (i + 1 >= nch) break;
      if (i + 2 < nch) store(i + 2, s1);
      if (i + 4 < nch) load(i + 4, s1);
      lds_barrier();
      if (i + 2 >= nch) break;
    }
    return;
  }

  // ---- compute waves: wave (wr, wc) owns row tiles wr TM .. and column tiles wc TN ..
  const int h = lane >> 5, l32 = lane & 31;
  const int wr = wave % WR, wc = wave / WR;
  const int ct0 = wc * TN;
  const bool active = ct0 * 32 < N;  // wave-uniform
  const int nks = K / 16;
  // filter fragment of tile b, step kg: chunk 2 kg + h of row n (columns past N: clamped, their
  // products are never stored)
  const u32x4* wb[TN];
#pragma unroll
  for (int b = 0; b < TN; ++b) {
    const int n = min((ct0 + b) * 32 + l32, N - 1);
    wb[b] = p.ws + ((long)n * (K / 8) + h) * 2;
  }
  auto load_b = [&](int kg, u32x4 (&bh)[TN], u32x4 (&bl)[TN]) {
#pragma unroll
    for (int b = 0; b < TN; ++b) {
      bh[b] = wb[b][4 * kg];
      bl[b] = wb[b][4 * kg + 1];
    }
  };
  floatx16 acc[TM][TN];
#pragma unroll
  for (int a = 0; a < TM; ++a)
#pragma unroll
    for (int b = 0; b < TN; ++b)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[a][b][r] = 0.f;
  u32x4 bh[TN], bl[TN], nh[TN], nl[TN];
  if (active) load_b(0, bh, bl);
  lds_barrier();
  for (int i = 0; i < nch; ++i) {
    if (active) {
      const unsigned char* img = smem + (i & 1) * BUF;
      const int ns = min(KC / 16, nks - (KC / 16) * i);
#pragma unroll
      for (int s = 0; s < KC / 16; ++s) {
        if (s < ns) {
          const int kg = (KC / 16) * i + s;
          load_b(min(kg + 1, nks - 1), nh, nl);
          bf16x8 ah[TM], al[TM];
#pragma unroll
          for (int a = 0; a < TM; ++a) {
            const int o = ((wr * TM + a) * 32 + l32) * RS + 32 * s + 16 * h;
            ah[a] = __builtin_bit_cast(bf16x8, *reinterpret_cast<const u32x4*>(img + o));
            al[a] = __builtin_bit_cast(bf16x8, *reinterpret_cast<const u32x4*>(img + PLANE + o));
          }
#pragma unroll
          for (int b = 0; b < TN; ++b) {
            const bf16x8 fh = __builtin_bit_cast(bf16x8, bh[b]);
            const bf16x8 fl = __builtin_bit_cast(bf16x8, bl[b]);
#pragma unroll
            for (int a = 0; a < TM; ++a) {
              acc[a][b] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(al[a], fh, acc[a][b], 0, 0, 0);
              acc[a][b] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ah[a], fl, acc[a][b], 0, 0, 0);
              acc[a][b] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ah[a], fh, acc[a][b], 0, 0, 0);
            }
          }
#pragma unroll
          for (int b = 0; b < TN; ++b) {
            bh[b] = nh[b];
            bl[b] = nl[b];
          }
        }
      }
    }
    lds_barrier();
  }
  if (!active) return;
  // every wave is past the last chunk: the A buffers are free and hold the output staging tiles.
  // Lane holds column l32, rows (r & 3) + 8 (r >> 2) + 4 h of a tile; it goes out as float4 row
  // segments (8 rows x 128 bytes per store instruction)
  float* ob = reinterpret_cast<float*>(smem) + wave * (32 * OLS);
#pragma unroll
  for (int a = 0; a < TM; ++a) {
    const long rs = m0 + (wr * TM + a) * 32;
#pragma unroll
    for (int b = 0; b < TN; ++b) {
      const int col0 = (ct0 + b) * 32;
      if (col0 >= N || rs >= M) continue;  // wave-uniform
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int rr = (r & 3) + 8 * (r >> 2) + 4 * h;
        const float v = acc[a][b][r];
        ob[rr * OLS + l32] = v;
      }
      __builtin_amdgcn_wave_barrier();
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
      const int cq = col0 + 4 * (lane & 7);
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int rr = (lane >> 3) + 8 * i;
        if (rs + rr < M && cq < N) {
          float4 v = *reinterpret_cast<const float4*>(ob + rr * OLS + 4 * (lane & 7));
          float4* d = reinterpret_cast<float4*>(p.y + (rs + rr) * N + cq);
          if (p.acc) v = add4(v, *d);
          *d = v;
        }
      }
      __builtin_amdgcn_wave_barrier();
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    }
  }
}

// The tiling is a function of the output width alone: all columns in one workgroup, 64-row
// strips while the accumulators of a wave stay at 32 VGPRs (N <= 128), 32-row strips beyond
// (N = 192 / 320 occur at 14 x 14 only: 6272 rows, 196 workgroups).
struct Plan {
  int cfg, bm;
};
static Plan plan(int N) {
  const int nt = (N + 31) / 32;
  if (nt <= 2) return {0, 64};   // TM 1, WR 2, TN 1
  if (nt <= 4) return {1, 64};   // TM 2, WR 1, TN 1
  if (nt <= 8) return {2, 32};   // TM 1, WR 1, TN 2
  return {3, 32};                // TM 1, WR 1, TN 3
}

template <int PRO>
static int launch(const Params& p, hipStream_t st) {
  const Plan pl = plan(p.N);
  const int nv = PRO == PRO_BNBWD ? 6 : 4;
  const unsigned grid = cdiv(p.M, pl.bm);
  const size_t prm = sizeof(float) * nv * p.K;
  constexpr int T = (NCW + NLW) * 64;
  switch (pl.cfg) {
    case 0:
      pgemm_x3_kernel<PRO, 1, 2, 1><<<grid, T, a_region_bytes<1, 2>() + prm, st>>>(p);
      break;
    case 1:
      pgemm_x3_kernel<PRO, 2, 1, 1><<<grid, T, a_region_bytes<2, 1>() + prm, st>>>(p);
      break;
    case 2:
      pgemm_x3_kernel<PRO, 1, 1, 2><<<grid, T, a_region_bytes<1, 1>() + prm, st>>>(p);
      break;
    default:
      pgemm_x3_kernel<PRO, 1, 1, 3><<<grid, T, a_region_bytes<1, 1>() + prm, st>>>(p);
      break;
  }
  return check_launch("pgemm_x3_kernel");
}

}  // namespace px3
}  // namespace pld

using namespace pld;

static bool px3_shape_ok(int k, int n) {
  return k >= 16 && k % 16 == 0 && k <= px3::K_MAX && n >= 4 && n % 4 == 0 && n <= px3::N_MAX;
}

// a status, as every int entry point: PLD_OK where the kernels take the shape
extern "C" int pld_pgemm_x3_ok(int k, int n) {
  PLD_CHECK_ARG(px3_shape_ok(k, n), "pld_pgemm_x3: K=%d N=%d unsupported (K %% 16 == 0, "
                "K <= %d, N %% 4 == 0, N <= %d)", k, n, px3::K_MAX, px3::N_MAX);
  return PLD_OK;
}

static int px3_check(const float* x, int64_t rows, int k, const float* mean, const float* invstd,
                     const float* gamma, const float* beta, const void* w_split, int n,
                     float* y) {
  PLD_CHECK_ARG(x && mean && invstd && gamma && beta && w_split && y && rows > 0,
                "pld_pgemm_x3: bad args");
  int rc = pld_pgemm_x3_ok(k, n);
  if (rc) return rc;
  PLD_CHECK_ARG(aligned16(x) && aligned16(mean) && aligned16(invstd) && aligned16(gamma) &&
                    aligned16(beta) && aligned16(w_split) && aligned16(y),
                "pld_pgemm_x3: operands must be 16-byte aligned");
  PLD_CHECK_ARG(rows * (int64_t)k < (1L << 31) && rows * (int64_t)n < (1L << 31),
                "pld_pgemm_x3: tensor too large");
  return PLD_OK;
}

extern "C" int pld_pgemm_x3_bn_act(const float* x, int64_t rows, int k, const float* mean,
                                   const float* invstd, const float* gamma, const float* beta,
                                   int act, const float* gate, int hw, const void* w_split,
                                   int n, float* y, int accumulate, void* stream) {
  int rc = px3_check(x, rows, k, mean, invstd, gamma, beta, w_split, n, y);
  if (rc) return rc;
  PLD_CHECK_ARG(!gate || (hw > 0 && aligned16(gate)), "pld_pgemm_x3_bn_act: gate needs hw > 0");
  px3::Params p{};
  p.x = x; p.mean = mean; p.invstd = invstd; p.gamma = gamma; p.beta = beta;
  p.gate = gate; p.ws = reinterpret_cast<const px3::u32x4*>(w_split); p.y = y;
  p.M = (int)rows; p.K = k; p.N = n; p.act = act; p.acc = accumulate;
  p.dHW = FastDiv((uint32_t)(hw > 0 ? hw : 1));
  return px3::launch<px3::PRO_BNACT>(p, as_stream(stream));
}

extern "C" int pld_pgemm_x3_bn_bwd(const float* x, const float* dy, int64_t rows, int k,
                                   const float* mean, const float* invstd, const float* gamma,
                                   const float* beta, int act, const float* k12,
                                   const void* w_split, int n, float* y, int accumulate,
                                   void* stream) {
  int rc = px3_check(x, rows, k, mean, invstd, gamma, beta, w_split, n, y);
  if (rc) return rc;
  PLD_CHECK_ARG(dy && k12 && aligned16(dy) && aligned16(k12),
                "pld_pgemm_x3_bn_bwd: bad dy / k12");
  px3::Params p{};
  p.x = x; p.dy = dy; p.mean = mean; p.invstd = invstd; p.gamma = gamma; p.beta = beta;
  p.k12 = k12; p.ws = reinterpret_cast<const px3::u32x4*>(w_split); p.y = y;
  p.M = (int)rows; p.K = k; p.N = n; p.act = act; p.acc = accumulate;
  return px3::launch<px3::PRO_BNBWD>(p, as_stream(stream));
}
