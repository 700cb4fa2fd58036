// Implicit-GEMM convolution on CDNA4 fp32 MFMA (v_mfma_f32_32x32x2_f32: exact fp32, a k-ordered
// fmaf chain — the only gfx950 matrix path that holds the 1e-3 fp32 parity bar of BASELINE.json).
//
// Replaces TF Conv2D / Conv2DBackpropInput / Conv2DBackpropFilter as Keras dispatches them for
//   * the ff_effnet decoder (pldepth/models/pl_hourglass.py:59-96: 3x3 'same' + bias, the
//     [x, skip] concatenations at :66,:75,:84 read as two sources — never materialised),
//   * EfficientNetB0's 1x1 expand/project/top convs and the 3x3/s2 stem (frozen: fwd + dX),
//   * the ReDWeb decoder / ResNet-50 convs (pldepth/models/redweb.py).
//
// Three GEMM views of one NHWC convolution, one kernel template:
//   FWD   : C[m=(img,oy,ox)][co]      = sum_{k=(ty,tx,ci)} X[img,oy*s+ty-pt,ox*s+tx-pl,ci] * Wn[co][k]
//   DGRAD : the same kernel with X := dY, Wn := flipped filter [ci][ty][tx][co] (stride 1 only);
//           output columns split between dx1 (channels < c1) and dx2 (concat source 2)
//   WGRAD : C[i=(ty,tx,ci)][co] = sum_{p=(img,oy,ox)} X[img,oy*s+ty-pt,ox*s+tx-pl,ci] * dY[p][co]
//           split-K over pixels into fp32 slabs, reduced in a fixed order (deterministic)
//
// Tiling: 256 threads = 4 waves, block tile BM x BN x 16; each wave owns (BM/WM) x (BN/WN) as
// 32x32 MFMA tiles. Operands are staged global -> registers -> LDS (double-buffered, one
// barrier per K-step; the next tile's global loads are issued before the current tile's MFMAs).
// The K index inside a 16-step is permuted (lane half h, step kk) -> k = 8h + kk for both
// operands, so each lane reads its 8 A (B) values of a step as two contiguous float4 from LDS.
// Roofline: MFMA-bound for the decoder shapes (fp32 peak 157.3 TF/s), HBM-bound for skinny
// encoder 1x1 convs (K = 16..40).
#include <algorithm>
#include <cstdio>
#include <cstdlib>

#include "conv_common.h"

namespace pld {

constexpr int BK = 16;
constexpr int PADK = 4;  // [row][BK+PADK]: 80-byte rows -> conflict-free b128 fragment reads

template <int BM, int BN, int WM, int WN, int MODE, bool VEC, bool VEC16>
__global__ __launch_bounds__(256) void conv_igemm_kernel(GemmConvParams p) {
  static_assert(WM * WN == 4, "4 waves");
  constexpr int WTM = BM / WM, WTN = BN / WN;
  constexpr int TM = WTM / 32, TN = WTN / 32;
  static_assert(TM >= 1 && TN >= 1, "wave tile >= 32x32");
  // LDS images. FWD: [row][BK+PADK] (k contiguous). WGRAD: [k][row+PADK] (row contiguous).
  constexpr int A_ELEMS = (MODE == MODE_FWD) ? BM * (BK + PADK) : BK * (BM + PADK);
  constexpr int B_ELEMS = (MODE == MODE_FWD) ? BN * (BK + PADK) : BK * (BN + PADK);
  __shared__ __attribute__((aligned(16))) float smem[2 * (A_ELEMS + B_ELEMS)];
#define As(buf) (smem + (buf) * A_ELEMS)
#define Bs(buf) (smem + 2 * A_ELEMS + (buf) * B_ELEMS)

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = tid >> 6;
  const int wm = wave / WN, wn = wave % WN;
  const int m0 = blockIdx.x * BM;
  const int n0 = blockIdx.y * BN;

  int kt_begin = 0, kt_end = (p.K + BK - 1) / BK;
  if (p.ktiles_per_split > 0) {  // split-K: this workgroup's slice of the reduction
    kt_begin = blockIdx.z * p.ktiles_per_split;
    kt_end = min(kt_end, kt_begin + p.ktiles_per_split);
  }

  // ------------------------------------------------------------------ descriptors
  // x1/x2 are addressed relative to the first image this workgroup touches, so offsets stay
  // 32-bit for any batch (the host bounds the span one workgroup can reach).
  int img_base, pix_base = 0;
  if (MODE == MODE_FWD) {
    img_base = (int)p.dOH.div(p.dOW.div((uint32_t)m0));
  } else {
    pix_base = kt_begin * BK;
    img_base = (int)p.dOH.div(p.dOW.div((uint32_t)min(pix_base, p.K - 1)));
  }
  const long img_elems = (long)p.h * p.w;
  const __amdgpu_buffer_rsrc_t rs1 =
      make_rsrc(p.x1 + img_base * img_elems * p.c1, (p.n - img_base) * img_elems * p.c1 * 4);
  const __amdgpu_buffer_rsrc_t rs2 =
      p.c2 ? make_rsrc(p.x2 + img_base * img_elems * p.c2, (p.n - img_base) * img_elems * p.c2 * 4)
           : make_rsrc(p.x1, 0);
  const __amdgpu_buffer_rsrc_t rsb =
      (MODE == MODE_FWD) ? make_rsrc(p.bmat, (long)p.N * p.K * 4)
                         : make_rsrc(p.bmat + (long)pix_base * p.N, (long)(p.K - pix_base) * p.N * 4);

  // ------------------------------------------------------------------ staging registers
  // FWD A: BM rows x 4 float4 ; thread -> (row = tid/4 + 64 j, kq = tid%4)
  // FWD B: BN rows x 4 float4 ; same mapping, rows < BN
  // WGRAD A: 16 k-rows x BM/4 float4 ; thread -> (krow = tid / (BM/4) + (256/(BM/4)) j, i4)
  // WGRAD B: 16 k-rows x BN/4 float4
  constexpr int A_V4 = BM * BK / 4, B_V4 = BN * BK / 4;
  constexpr int A_PER = (A_V4 + 255) / 256, B_PER = (B_V4 + 255) / 256;
  constexpr bool DUAL = !VEC16;  // separate source-2 staging (concat whose K-steps mix sources)
  float4 ra[A_PER], rb[B_PER];
  float4 ra2[DUAL ? A_PER : 1];
  unsigned vmask = 0;  // valid (in-image) elements of the staged A tile: prologue targets
  unsigned pmask = 0;  // elements from source 1 (prologue applies) — scalar paths
  float4 psc = make_float4(0.f, 0.f, 0.f, 0.f), psh = psc;  // prologue scale/shift (VEC paths)
  float esc[4] = {0.f, 0.f, 0.f, 0.f}, esh[4] = {0.f, 0.f, 0.f, 0.f};  // (scalar paths)
  bool pro = false;
  const int kq = tid & 3;

  // per-thread constants. FWD: pixel decomposition of this thread's A rows
  int a_ir[A_PER], a_iy0[A_PER], a_ix0[A_PER];
  bool a_ok[A_PER];
  // WGRAD: tap/channel decomposition of this thread's A column group (per element when !VEC)
  int w_ty[4], w_tx[4], w_ci[4];
  bool w_ok[4];
  if (MODE == MODE_FWD) {
#pragma unroll
    for (int j = 0; j < A_PER; ++j) {
      const int v = tid + 256 * j;
      const int m = m0 + v / 4;
      a_ok[j] = (v < A_V4) && (m < p.M);
      const int mm = a_ok[j] ? m : m0;
      const uint32_t q = p.dOW.div((uint32_t)mm);
      const int ox = mm - (int)q * p.ow;
      const uint32_t img = p.dOH.div(q);
      const int oy = (int)q - (int)img * p.oh;
      a_ir[j] = ((int)img - img_base) * p.h;
      a_iy0[j] = oy * p.sh - p.pt;
      a_ix0[j] = ox * p.sw - p.pl;
    }
  } else {
    const int i0 = m0 + 4 * (tid % (BM / 4));
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int i = i0 + (VEC ? 0 : u);
      w_ok[u] = i < p.M;
      const int ii = w_ok[u] ? i : 0;
      const uint32_t tap = p.dC.div((uint32_t)ii);
      w_ci[u] = ii - (int)tap * p.C;
      const uint32_t ty = p.dKW.div(tap);
      w_ty[u] = (int)ty;
      w_tx[u] = (int)tap - (int)ty * p.kw;
    }
    if (p.in_scale) {  // a thread's channels are fixed in WGRAD: fetch the prologue once
      if (VEC) {
        pro = w_ok[0] && w_ci[0] < p.c1;
        if (pro) {
          psc = *reinterpret_cast<const float4*>(p.in_scale + w_ci[0]);
          psh = *reinterpret_cast<const float4*>(p.in_shift + w_ci[0]);
        }
      } else {
        pro = true;
#pragma unroll
        for (int u = 0; u < 4; ++u)
          if (w_ok[u] && w_ci[u] < p.c1) {
            esc[u] = p.in_scale[w_ci[u]];
            esh[u] = p.in_shift[w_ci[u]];
          }
      }
    }
  }

  auto load_tile = [&](int kt) {
    const int k0 = kt * BK;
    vmask = 0;
    pmask = 0;
    if (MODE == MODE_FWD) {
      if (VEC16) {
        // C % 16 == 0 and c1 % 16 == 0: the whole 16-wide K-step sits in one tap and one source;
        // its decomposition (and the descriptor choice) is wave-uniform
        const int tap = (int)p.dC.div((uint32_t)k0);
        const int ci = k0 - tap * p.C;
        const int ty = (int)p.dKW.div((uint32_t)tap);
        const int tx = tap - ty * p.kw;
        const bool src2 = ci >= p.c1;
        const int cs = src2 ? p.c2 : p.c1;
        const int cb = (src2 ? ci - p.c1 : ci) + 4 * kq;
        const __amdgpu_buffer_rsrc_t rs = src2 ? rs2 : rs1;
#pragma unroll
        for (int j = 0; j < A_PER; ++j) {
          const int iy = a_iy0[j] + ty, ix = a_ix0[j] + tx;
          const bool ok = a_ok[j] && (unsigned)iy < (unsigned)p.h && (unsigned)ix < (unsigned)p.w;
          const unsigned off = ok ? (unsigned)((((a_ir[j] + iy) * p.w + ix) * cs + cb) * 4) : OOB;
          ra[j] = bload4(rs, off);
          vmask |= (unsigned)ok << j;
        }
        pro = p.in_scale && !src2;
        if (pro) {
          psc = *reinterpret_cast<const float4*>(p.in_scale + cb);
          psh = *reinterpret_cast<const float4*>(p.in_shift + cb);
        }
      } else if (VEC) {
        const int k = k0 + 4 * kq;
        const bool kin = k < p.K;
        const int kk = kin ? k : 0;
        const int tap = (int)p.dC.div((uint32_t)kk);
        const int ci = kk - tap * p.C;
        const int ty = (int)p.dKW.div((uint32_t)tap);
        const int tx = tap - ty * p.kw;
        const bool in1 = ci < p.c1;
#pragma unroll
        for (int j = 0; j < A_PER; ++j) {
          const int iy = a_iy0[j] + ty, ix = a_ix0[j] + tx;
          const bool ok = kin && a_ok[j] && (unsigned)iy < (unsigned)p.h &&
                          (unsigned)ix < (unsigned)p.w;
          const int pix = (a_ir[j] + iy) * p.w + ix;
          ra[j] = bload4(rs1, (ok && in1) ? (unsigned)((pix * p.c1 + ci) * 4) : OOB);
          if (p.c2)
            ra2[j] = bload4(rs2, (ok && !in1) ? (unsigned)((pix * p.c2 + ci - p.c1) * 4) : OOB);
          vmask |= (unsigned)ok << j;
        }
        pro = p.in_scale && kin && in1;
        if (pro) {
          psc = *reinterpret_cast<const float4*>(p.in_scale + ci);
          psh = *reinterpret_cast<const float4*>(p.in_shift + ci);
        }
      } else {
        int ty[4], tx[4], ci[4];
        bool kin[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
          const int k = k0 + 4 * kq + u;
          kin[u] = k < p.K;
          const int kk = kin[u] ? k : 0;
          const int tap = (int)p.dC.div((uint32_t)kk);
          ci[u] = kk - tap * p.C;
          ty[u] = (int)p.dKW.div((uint32_t)tap);
          tx[u] = tap - ty[u] * p.kw;
          pmask |= (unsigned)(kin[u] && ci[u] < p.c1) << u;
          if (p.in_scale && kin[u] && ci[u] < p.c1) {
            esc[u] = p.in_scale[ci[u]];
            esh[u] = p.in_shift[ci[u]];
          }
        }
#pragma unroll
        for (int j = 0; j < A_PER; ++j) {
          float e1[4], e2[4];
#pragma unroll
          for (int u = 0; u < 4; ++u) {
            const int iy = a_iy0[j] + ty[u], ix = a_ix0[j] + tx[u];
            const bool ok = kin[u] && a_ok[j] && (unsigned)iy < (unsigned)p.h &&
                            (unsigned)ix < (unsigned)p.w;
            const int pix = (a_ir[j] + iy) * p.w + ix;
            const bool in1 = ci[u] < p.c1;
            e1[u] = bload1(rs1, (ok && in1) ? (unsigned)((pix * p.c1 + ci[u]) * 4) : OOB);
            e2[u] = p.c2 ? bload1(rs2, (ok && !in1) ? (unsigned)((pix * p.c2 + ci[u] - p.c1) * 4)
                                                    : OOB)
                         : 0.f;
            vmask |= (unsigned)ok << (4 * j + u);
          }
          ra[j] = make_float4(e1[0], e1[1], e1[2], e1[3]);
          ra2[j] = make_float4(e2[0], e2[1], e2[2], e2[3]);
        }
        pro = p.in_scale != nullptr;
      }
#pragma unroll
      for (int j = 0; j < B_PER; ++j) {
        const int v = tid + 256 * j;
        const int row = v >> 2;
        const int n = n0 + row;
        const int k = k0 + 4 * kq;
        const bool nok = v < B_V4 && n < p.N;
        if (VEC) {
          rb[j] = bload4(rsb, (nok && k < p.K) ? (unsigned)((n * p.K + k) * 4) : OOB);
        } else {
          float e[4];
#pragma unroll
          for (int u = 0; u < 4; ++u)
            e[u] = bload1(rsb, (nok && k + u < p.K) ? (unsigned)((n * p.K + k + u) * 4) : OOB);
          rb[j] = make_float4(e[0], e[1], e[2], e[3]);
        }
      }
    } else {  // WGRAD
      constexpr int AQ = BM / 4;  // float4 per k-row
#pragma unroll
      for (int j = 0; j < A_PER; ++j) {
        const int krow = (tid + 256 * j) / AQ;
        const int pix = k0 + krow;
        const bool rok = krow < BK && pix < p.K;
        const int pp = rok ? pix : pix_base;
        const uint32_t q = p.dOW.div((uint32_t)pp);
        const int ox = pp - (int)q * p.ow;
        const uint32_t img = p.dOH.div(q);
        const int oy = (int)q - (int)img * p.oh;
        const int ir = ((int)img - img_base) * p.h;
        if (VEC) {
          const int iy = oy * p.sh - p.pt + w_ty[0], ix = ox * p.sw - p.pl + w_tx[0];
          const bool ok = rok && w_ok[0] && (unsigned)iy < (unsigned)p.h &&
                          (unsigned)ix < (unsigned)p.w;
          const int px = (ir + iy) * p.w + ix;
          const bool in1 = w_ci[0] < p.c1;
          ra[j] = bload4(rs1, (ok && in1) ? (unsigned)((px * p.c1 + w_ci[0]) * 4) : OOB);
          if (p.c2)
            ra2[j] = bload4(rs2, (ok && !in1) ? (unsigned)((px * p.c2 + w_ci[0] - p.c1) * 4)
                                              : OOB);
          vmask |= (unsigned)ok << j;
        } else {
          float e1[4], e2[4];
#pragma unroll
          for (int u = 0; u < 4; ++u) {
            const int iy = oy * p.sh - p.pt + w_ty[u], ix = ox * p.sw - p.pl + w_tx[u];
            const bool ok = rok && w_ok[u] && (unsigned)iy < (unsigned)p.h &&
                            (unsigned)ix < (unsigned)p.w;
            const int px = (ir + iy) * p.w + ix;
            const bool in1 = w_ci[u] < p.c1;
            e1[u] = bload1(rs1, (ok && in1) ? (unsigned)((px * p.c1 + w_ci[u]) * 4) : OOB);
            e2[u] = p.c2 ? bload1(rs2, (ok && !in1) ? (unsigned)((px * p.c2 + w_ci[u] - p.c1) * 4)
                                                    : OOB)
                         : 0.f;
            vmask |= (unsigned)ok << (4 * j + u);
          }
          ra[j] = make_float4(e1[0], e1[1], e1[2], e1[3]);
          ra2[j] = make_float4(e2[0], e2[1], e2[2], e2[3]);
        }
      }
      constexpr int BQ = BN / 4;
#pragma unroll
      for (int j = 0; j < B_PER; ++j) {
        // linear float4 slot v -> (k-row, column quad): covers all BK x BQ slots for any BN
        const int krow = (tid + 256 * j) / BQ;
        const int pix = k0 + krow;
        const int n = n0 + 4 * ((tid + 256 * j) % BQ);
        const bool rok = krow < BK && pix < p.K;
        const int rel = (pix - pix_base) * p.N + n;
        if ((p.N & 3) == 0) {
          rb[j] = bload4(rsb, (rok && n < p.N) ? (unsigned)(rel * 4) : OOB);
        } else {
          float e[4];
#pragma unroll
          for (int u = 0; u < 4; ++u)
            e[u] = bload1(rsb, (rok && n + u < p.N) ? (unsigned)((rel + u) * 4) : OOB);
          rb[j] = make_float4(e[0], e[1], e[2], e[3]);
        }
      }
    }
  };

  // staged A value for LDS: the prologue act(x*scale+shift) on in-image source-1 elements
  // (padding taps stay 0: TF pads the activated tensor), plus the source-2 part
  auto finish_a = [&](int j) -> float4 {
    float4 v = ra[j];
    if (VEC) {
      if (pro && ((vmask >> j) & 1u)) v = prologue4(p.in_act, v, psc, psh);
    } else {
      if (pro) {
        float e[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
        for (int u = 0; u < 4; ++u) {
          const unsigned bit = (MODE == MODE_FWD) ? ((pmask >> u) & 1u)
                                                  : (unsigned)(w_ok[u] && w_ci[u] < p.c1);
          if (bit && ((vmask >> (4 * j + u)) & 1u))
            e[u] = act_fwd(p.in_act, e[u] * esc[u] + esh[u]);
        }
        v = make_float4(e[0], e[1], e[2], e[3]);
      }
    }
    if constexpr (DUAL) {
      if (p.c2) v = add4(v, ra2[j]);
    }
    return v;
  };

  auto store_tile = [&](int buf) {
    if (MODE == MODE_FWD) {
#pragma unroll
      for (int j = 0; j < A_PER; ++j) {
        const int v = tid + 256 * j;
        if (v < A_V4)
          *reinterpret_cast<float4*>(As(buf) + (v >> 2) * (BK + PADK) + 4 * (v & 3)) =
              finish_a(j);
      }
#pragma unroll
      for (int j = 0; j < B_PER; ++j) {
        const int v = tid + 256 * j;
        if (v < B_V4)
          *reinterpret_cast<float4*>(Bs(buf) + (v >> 2) * (BK + PADK) + 4 * (v & 3)) = rb[j];
      }
    } else {
      constexpr int AQ = BM / 4;
#pragma unroll
      for (int j = 0; j < A_PER; ++j) {
        const int v = tid + 256 * j;
        if (v / AQ < BK)
          *reinterpret_cast<float4*>(As(buf) + (v / AQ) * (BM + PADK) + 4 * (v % AQ)) = finish_a(j);
      }
      constexpr int BQ = BN / 4;
#pragma unroll
      for (int j = 0; j < B_PER; ++j) {
        const int v = tid + 256 * j;
        if (v / BQ < BK)
          *reinterpret_cast<float4*>(Bs(buf) + (v / BQ) * (BN + PADK) + 4 * (v % BQ)) = rb[j];
      }
    }
  };

  floatx16 acc[TM][TN];
#pragma unroll
  for (int a = 0; a < TM; ++a)
#pragma unroll
    for (int b = 0; b < TN; ++b)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[a][b][r] = 0.f;

  const int h = lane >> 5;
  const int l32 = lane & 31;

  if (kt_begin < kt_end) {
    load_tile(kt_begin);
    store_tile(0);
  }
  __syncthreads();
  for (int kt = kt_begin; kt < kt_end; ++kt) {
    const int buf = (kt - kt_begin) & 1;
    // the next tile's loads issue unconditionally (the last step re-fetches its own tile into
    // the idle buffer): no loop-carried select on the staging registers, so nothing waits on
    // the loads until store_tile after the MFMAs
    load_tile(kt + 1 < kt_end ? kt + 1 : kt);
    const float* A = As(buf);
    const float* Bm = Bs(buf);
    float af[TM][8], bf[TN][8];
    if (MODE == MODE_FWD) {
#pragma unroll
      for (int a = 0; a < TM; ++a) {
        const float* src = A + (wm * WTM + a * 32 + l32) * (BK + PADK) + 8 * h;
        const float4 lo = *reinterpret_cast<const float4*>(src);
        const float4 hi = *reinterpret_cast<const float4*>(src + 4);
        af[a][0] = lo.x; af[a][1] = lo.y; af[a][2] = lo.z; af[a][3] = lo.w;
        af[a][4] = hi.x; af[a][5] = hi.y; af[a][6] = hi.z; af[a][7] = hi.w;
      }
#pragma unroll
      for (int b = 0; b < TN; ++b) {
        const float* src = Bm + (wn * WTN + b * 32 + l32) * (BK + PADK) + 8 * h;
        const float4 lo = *reinterpret_cast<const float4*>(src);
        const float4 hi = *reinterpret_cast<const float4*>(src + 4);
        bf[b][0] = lo.x; bf[b][1] = lo.y; bf[b][2] = lo.z; bf[b][3] = lo.w;
        bf[b][4] = hi.x; bf[b][5] = hi.y; bf[b][6] = hi.z; bf[b][7] = hi.w;
      }
    } else {
#pragma unroll
      for (int kk = 0; kk < 8; ++kk) {
#pragma unroll
        for (int a = 0; a < TM; ++a)
          af[a][kk] = A[(8 * h + kk) * (BM + PADK) + wm * WTM + a * 32 + l32];
#pragma unroll
        for (int b = 0; b < TN; ++b)
          bf[b][kk] = Bm[(8 * h + kk) * (BN + PADK) + wn * WTN + b * 32 + l32];
      }
    }
#pragma unroll
    for (int kk = 0; kk < 8; ++kk)
#pragma unroll
      for (int a = 0; a < TM; ++a)
#pragma unroll
        for (int b = 0; b < TN; ++b)
          acc[a][b] = __builtin_amdgcn_mfma_f32_32x32x2f32(af[a][kk], bf[b][kk], acc[a][b], 0, 0, 0);
    store_tile(buf ^ 1);
    __syncthreads();
  }

#undef As
#undef Bs
  // the loop's last barrier has passed: the staging LDS is free, one region per wave
  if constexpr (4 * 32 * (WTN + 8) <= 2 * (A_ELEMS + B_ELEMS)) {
    if (staged_ok(p)) {
      if (p.stats) acc_stats<TM, TN>(p, acc, m0 + wm * WTM, n0 + wn * WTN, lane);
      store_acc_staged<TM, TN>(p, acc, m0 + wm * WTM, n0 + wn * WTN, lane,
                               smem + wave * 32 * (WTN + 8));
      return;
    }
  }
  store_acc<TM, TN>(p, acc, m0 + wm * WTM, n0 + wn * WTN, lane);
}

// ordered split-K reduction: dw[i] (+)= sum_z ws[z][i]
__global__ __launch_bounds__(256) void splitk_reduce_kernel(const float* __restrict__ ws,
                                                            int splits, long n,
                                                            float* __restrict__ dw, int acc) {
  const long stride = (long)gridDim.x * blockDim.x;
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
    float s = 0.f;
    for (int z = 0; z < splits; ++z) s += ws[(long)z * n + i];
    dw[i] = acc ? dw[i] + s : s;
  }
}

// first level of a two-level ordered reduction for many split-K slabs: group g sums slabs
// [g*per, (g+1)*per) in order into part[g][i] (enough threads when M*N is small and splits many)
constexpr int SPLIT_GROUP = 16;

__global__ __launch_bounds__(256) void splitk_group_kernel(const float* __restrict__ ws,
                                                           int splits, long n,
                                                           float* __restrict__ part) {
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const int z0 = blockIdx.y * SPLIT_GROUP, z1 = min(splits, z0 + SPLIT_GROUP);
  float s = 0.f;
  for (int z = z0; z < z1; ++z) s += ws[(long)z * n + i];
  part[(long)blockIdx.y * n + i] = s;
}

// both levels of that reduction in one launch, in the same order (group g sums its SPLIT_GROUP
// slabs in order; the groups are then summed in order): a 256-thread block is EL elements x G
// group lanes (G = the group count rounded up to a power of two <= 32), the group sums meet in
// LDS. Bit-identical to splitk_group_kernel + splitk_reduce_kernel, one dependent launch less.
template <int G>
__global__ __launch_bounds__(256) void splitk_reduce2_kernel(const float* __restrict__ ws,
                                                             int splits, long n,
                                                             float* __restrict__ dw, int acc) {
  constexpr int EL = 256 / G;
  __shared__ float red[G][EL];
  const int e = threadIdx.x % EL, g = threadIdx.x / EL;
  const long i = (long)blockIdx.x * EL + e;
  const int groups = (splits + SPLIT_GROUP - 1) / SPLIT_GROUP;
  float s = 0.f;
  if (i < n && g < groups) {
    const int z1 = min(splits, (g + 1) * SPLIT_GROUP);
    for (int z = g * SPLIT_GROUP; z < z1; ++z) s += ws[(long)z * n + i];
  }
  red[g][e] = s;
  __syncthreads();
  if (g == 0 && i < n) {
    float t = 0.f;
    for (int k = 0; k < groups; ++k) t += red[k][e];
    dw[i] = acc ? dw[i] + t : t;
  }
}

// ordered split-K reduction of forward / dgrad slabs with bias and two-destination routing
__global__ __launch_bounds__(256) void splitk_out_kernel(const float* __restrict__ ws, int splits,
                                                         long M, int N, const float* bias,
                                                         float* out1, int ld1, int acc1,
                                                         float* out2, int ld2, int acc2,
                                                         int split) {
  const long n = M * N;
  const long stride = (long)gridDim.x * blockDim.x;
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
    float s = 0.f;
    for (int z = 0; z < splits; ++z) s += ws[(long)z * n + i];
    const long row = i / N;
    const int col = (int)(i - row * N);
    if (bias) s += bias[col];
    if (col < split) {
      float* d = out1 + row * ld1 + col;
      *d = acc1 ? *d + s : s;
    } else {
      float* d = out2 + row * ld2 + (col - split);
      *d = acc2 ? *d + s : s;
    }
  }
}

// strided 1x1 dgrad: dx[img][y][x][c] = (y%sh==0 && x%sw==0) ? t[img][y/sh][x/sw][c] : 0, with
// the channel range split across two destinations (concat inputs)
__global__ __launch_bounds__(256) void stride_scatter_kernel(const float* __restrict__ t, int n,
                                                             int h, int w, int oh, int ow,
                                                             int sh, int sw, int C,
                                                             float* out1, int c1, int acc1,
                                                             float* out2, int acc2) {
  const long total = (long)n * h * w * C;
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < total;
       i += (long)gridDim.x * blockDim.x) {
    const int c = (int)(i % C);
    long pix = i / C;
    const int x = (int)(pix % w);
    pix /= w;
    const int y = (int)(pix % h);
    const long img = pix / h;
    float v = 0.f;
    if (y % sh == 0 && x % sw == 0 && y / sh < oh && x / sw < ow)
      v = t[((img * oh + y / sh) * ow + x / sw) * C + c];
    const long px = (img * h + y) * w + x;
    if (c < c1) {
      float* d = out1 + px * c1 + c;
      *d = acc1 ? *d + v : v;
    } else {
      const int c2 = C - c1;
      float* d = out2 + px * c2 + (c - c1);
      *d = acc2 ? *d + v : v;
    }
  }
}

// The same with 4 channels per thread and 32-bit magic-number division (C, c1 % 4 == 0,
// 16-byte aligned buffers, < 2^31 elements): one (pixel, channel quad) per trip, the quad read
// only at the stride grid's pixels — the generic form's three 64-bit div/mod per element bound
// it by the ALU at ~2.4 TB/s
__global__ __launch_bounds__(256) void stride_scatter4_kernel(const float* __restrict__ t,
                                                              int total4, FastDiv dC4,
                                                              FastDiv dW, FastDiv dH, int oh,
                                                              int ow, int sh, int sw, int C,
                                                              float* out1, int c1, int acc1,
                                                              float* out2, int acc2) {
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < total4; i += gridDim.x * blockDim.x) {
    const uint32_t pix = dC4.div((uint32_t)i);
    const int c = 4 * (i - (int)pix * (int)dC4.d);
    const uint32_t r = dW.div(pix);
    const int x = (int)(pix - r * dW.d);
    const uint32_t img = dH.div(r);
    const int y = (int)(r - img * dH.d);
    float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
    const int ys = y / sh, xs = x / sw;
    if (y - ys * sh == 0 && x - xs * sw == 0 && ys < oh && xs < ow)
      v = *reinterpret_cast<const float4*>(t + (((long)img * oh + ys) * ow + xs) * C + c);
    float4* d;
    int acc;
    if (c < c1) {
      d = reinterpret_cast<float4*>(out1 + (long)pix * c1 + c);
      acc = acc1;
    } else {
      d = reinterpret_cast<float4*>(out2 + (long)pix * (C - c1) + (c - c1));
      acc = acc2;
    }
    if (acc) {
      const float4 o = *d;
      v = make_float4(o.x + v.x, o.y + v.y, o.z + v.z, o.w + v.w);
    }
    *d = v;
  }
}

// the accumulate form (every destination += t): only the stride grid's pixels change, so the
// walk is over t's [n][oh][ow][C / 4] quads (read t, read-modify-write one destination quad):
// a quarter of the input-resolution traffic of the full-grid form at stride 2
__global__ __launch_bounds__(256) void stride_scatter4_acc_kernel(const float* __restrict__ t,
                                                                  int total4, FastDiv dC4,
                                                                  FastDiv dOW, FastDiv dOH, int h,
                                                                  int w, int sh, int sw, int C,
                                                                  float* out1, int c1,
                                                                  float* out2) {
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < total4; i += gridDim.x * blockDim.x) {
    const uint32_t opix = dC4.div((uint32_t)i);
    const int c = 4 * (i - (int)opix * (int)dC4.d);
    const uint32_t r = dOW.div(opix);
    const int xs = (int)(opix - r * dOW.d);
    const uint32_t img = dOH.div(r);
    const int ys = (int)(r - img * dOH.d);
    const int y = ys * sh, x = xs * sw;
    if (y >= h || x >= w) continue;
    const long pix = ((long)img * h + y) * w + x;
    const float4 v = *reinterpret_cast<const float4*>(t + (long)opix * C + c);
    float4* d = c < c1 ? reinterpret_cast<float4*>(out1 + pix * c1 + c)
                       : reinterpret_cast<float4*>(out2 + pix * (C - c1) + (c - c1));
    const float4 o = *d;
    *d = make_float4(o.x + v.x, o.y + v.y, o.z + v.z, o.w + v.w);
  }
}

// HWIO [kh][kw][ci][co] -> [co][kh][kw][ci]
__global__ void filter_native_kernel(const float* __restrict__ w, int taps, int cin, int cout,
                                     float* __restrict__ o) {
  const long n = (long)taps * cin * cout;
  for (long e = (long)blockIdx.x * blockDim.x + threadIdx.x; e < n;
       e += (long)gridDim.x * blockDim.x) {
    const int co = (int)(e % cout);
    const long r = e / cout;  // = tap*cin + ci
    o[(long)co * taps * cin + r] = w[e];
  }
}

// HWIO -> [ci][kh'][kw'][co], kh' = kh-1-ty, kw' = kw-1-tx
__global__ void filter_dgrad_kernel(const float* __restrict__ w, int kh, int kw, int cin,
                                    int cout, float* __restrict__ o) {
  const long n = (long)kh * kw * cin * cout;
  for (long e = (long)blockIdx.x * blockDim.x + threadIdx.x; e < n;
       e += (long)gridDim.x * blockDim.x) {
    const int co = (int)(e % cout);
    long r = e / cout;
    const int ci = (int)(r % cin);
    r /= cin;
    const int tx = (int)(r % kw);
    const int ty = (int)(r / kw);
    const int fy = kh - 1 - ty, fx = kw - 1 - tx;
    o[(((long)ci * kh + fy) * kw + fx) * cout + co] = w[e];
  }
}

// ---- per-step filter refresh (trainable convs after the optimizer): both native layouts and
// their bf16x3 splits from the HWIO weights in two coalesced passes
typedef unsigned int u32x4r __attribute__((ext_vector_type(4)));

// 8 fp32 -> the pld_filter_split chunk: 8 bf16 hi then 8 bf16 lo (conv_x3.hip's split2)
__device__ __forceinline__ void split_chunk(const float* v, u32x4r* out) {
  unsigned hs[4], ls[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const __bf16 h0 = (__bf16)v[2 * i], h1 = (__bf16)v[2 * i + 1];
    const __bf16 l0 = (__bf16)(v[2 * i] - (float)h0), l1 = (__bf16)(v[2 * i + 1] - (float)h1);
    hs[i] = __builtin_bit_cast(unsigned short, h0) |
            (unsigned)__builtin_bit_cast(unsigned short, h1) << 16;
    ls[i] = __builtin_bit_cast(unsigned short, l0) |
            (unsigned)__builtin_bit_cast(unsigned short, l1) << 16;
  }
  out[0] = u32x4r{hs[0], hs[1], hs[2], hs[3]};
  out[1] = u32x4r{ls[0], ls[1], ls[2], ls[3]};
}

// HWIO viewed as W[R = taps*cin][cout] -> native O[cout][R]: 64x64 tiles transposed through LDS
// (row pitch 65: conflict-free both ways); every output lane writes one 8-value chunk (32 B of
// fp32 + its 32-B split). R % 8 == 0.
__device__ __forceinline__ void filter_native_tile(const float* __restrict__ w, int R, int cout,
                                                   float* __restrict__ o,
                                                   u32x4r* __restrict__ osplit, int bx, int by) {
  __shared__ float t[64][65];
  const int r0 = bx * 64, c0 = by * 64;
  const int tid = threadIdx.x, lc = tid & 63;
#pragma unroll
  for (int i = 0; i < 16; ++i) {
    const int r = (tid >> 6) + 4 * i, gr = r0 + r, gc = c0 + lc;
    t[lc][r] = (gr < R && gc < cout) ? w[(long)gr * cout + gc] : 0.f;
  }
  __syncthreads();
#pragma unroll
  for (int i = 0; i < 2; ++i) {
    const int e = tid + 256 * i, c = e >> 3, q = e & 7;
    const int gc = c0 + c, gr = r0 + 8 * q;
    if (gc < cout && gr < R) {
      float v[8];
#pragma unroll
      for (int j = 0; j < 8; ++j) v[j] = t[c][8 * q + j];
      const long f = (long)gc * R + gr;
      reinterpret_cast<float4*>(o + f)[0] = make_float4(v[0], v[1], v[2], v[3]);
      reinterpret_cast<float4*>(o + f)[1] = make_float4(v[4], v[5], v[6], v[7]);
      if (osplit) split_chunk(v, osplit + f / 4);
    }
  }
}

__global__ __launch_bounds__(256) void filter_native_tiled_kernel(const float* __restrict__ w,
                                                                  int R, int cout,
                                                                  float* __restrict__ o,
                                                                  u32x4r* __restrict__ osplit) {
  filter_native_tile(w, R, cout, o, osplit, blockIdx.x, blockIdx.y);
}

// HWIO -> dgrad [cin][taps'][cout] (taps flipped): a permutation of cout-long rows, one 8-value
// chunk per thread (coalesced both sides). cout % 8 == 0. Block b of nb.
__device__ __forceinline__ void filter_dgrad_rows(const float* __restrict__ w, int taps, int cin,
                                                  int cout, float* __restrict__ o,
                                                  u32x4r* __restrict__ osplit, int b, int nb) {
  const int c8n = cout >> 3;
  const long n = (long)cin * taps * c8n;
  for (long e = (long)b * 256 + threadIdx.x; e < n; e += (long)nb * 256) {
    const int c8 = (int)(e % c8n);
    const long rest = e / c8n;
    const int tp = (int)(rest % taps), ci = (int)(rest / taps);
    const float4* src = reinterpret_cast<const float4*>(
        w + ((long)(taps - 1 - tp) * cin + ci) * cout + 8 * c8);
    const float4 a = src[0], b = src[1];
    const long f = ((long)ci * taps + tp) * cout + 8 * c8;
    reinterpret_cast<float4*>(o + f)[0] = a;
    reinterpret_cast<float4*>(o + f)[1] = b;
    if (osplit) {
      const float v[8] = {a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w};
      split_chunk(v, osplit + f / 4);
    }
  }
}

__global__ __launch_bounds__(256) void filter_dgrad_rows_kernel(const float* __restrict__ w,
                                                                int taps, int cin, int cout,
                                                                float* __restrict__ o,
                                                                u32x4r* __restrict__ osplit) {
  filter_dgrad_rows(w, taps, cin, cout, o, osplit, blockIdx.x, gridDim.x);
}

// Every trainable conv's refresh in one launch: a flat grid over a device table of filters, each
// owning a contiguous block range (its native tiles, then its dgrad row blocks); a block finds
// its filter by a wave-uniform scan of the range starts. Same bytes as pld_filter_refresh.
static unsigned refresh_dgrad_blocks(long n8) { return std::min<unsigned>(cdiv(n8, 256), 8192); }

__global__ __launch_bounds__(256) void filter_refresh_multi_kernel(
    const pld_filter_refresh_desc* __restrict__ d, int count) {
  const int b = blockIdx.x;
  int i = 0;
  while (i + 1 < count && d[i + 1].blk0 <= b) ++i;
  const pld_filter_refresh_desc f = d[i];
  const int R = f.taps * f.cin;
  const int tx = (R + 63) / 64;
  const int nat = tx * ((f.cout + 63) / 64);
  const int lb = b - f.blk0;
  if (lb < nat)
    filter_native_tile(f.w, R, f.cout, f.w_nat, (u32x4r*)f.w_nat_split, lb % tx, lb / tx);
  else if (f.w_dgrad)
    filter_dgrad_rows(f.w, f.taps, f.cin, f.cout, f.w_dgrad, (u32x4r*)f.w_dgrad_split, lb - nat,
                      f.nblk - nat);
}

// ------------------------------------------------------------------------ dispatch
// ---- tile configurations and a small cost model ----
// (BM, BN, WM, WN): 4 waves; each wave computes (BM/WM) x (BN/WN) as 32x32 MFMA tiles.
// occ: resident blocks per CU (VGPR/AGPR bound, from the compiler's resource report)
struct TileCfg { int bm, bn, tm, tn, occ; };
static const TileCfg kTiles[] = {
    {256, 32, 2, 1, 3},  {128, 64, 1, 1, 4},  {128, 96, 1, 3, 4},  {128, 128, 2, 2, 3},
    {128, 160, 1, 5, 2}, {128, 192, 1, 6, 2}, {128, 224, 1, 7, 2}, {256, 64, 2, 2, 3},
    {256, 128, 4, 2, 1},
};

// estimated relative time: padded MFMA work per block x waves of blocks over 256 CUs,
// discounted by the per-wave tile count (fragment reuse)
static constexpr int kNumCfg = (int)(sizeof(kTiles) / sizeof(kTiles[0]));
static constexpr int kNumTiles = 2 * kNumCfg;  // x {no split-K, split-K} for fwd / dgrad

static int choose_tile(long M, long N, long K, int splits, int requested = -1) {
  if (requested >= 0 && requested < kNumTiles) return requested % kNumCfg;
  // measurement override (tile sweeps): PLD_CONV_TILE=<index into kTiles>
  static const char* ov = getenv("PLD_CONV_TILE");
  if (ov && *ov) return atoi(ov);
  int best = 0;
  double best_t = 1e300;
  for (int i = 0; i < kNumCfg; ++i) {
    const TileCfg& t = kTiles[i];
    const long blocks = (long)cdiv(M, t.bm) * cdiv(N, t.bn) * splits;
    const int per_wave = t.tm * t.tn;
    const double eff = per_wave >= 4 ? 1.0 : (per_wave == 3 ? 0.9 : (per_wave == 2 ? 0.8 : 0.55));
    const int occ = t.occ;
    const double rounds = std::ceil((double)blocks / (256.0 * occ));
    const double t_est = rounds * occ * (double)t.bm * t.bn * ((double)K / splits) / eff;
    if (t_est < best_t * 0.97) {
      best_t = t_est;
      best = i;
    }
  }
  return best;
}

template <int MODE, int BM, int BN, int WM, int WN>
static void launch_cfg(GemmConvParams& p, bool vec, bool vec16, int splits, hipStream_t st) {
  dim3 grid(cdiv(p.M, BM), cdiv(p.N, BN), splits);
  if (vec16) conv_igemm_kernel<BM, BN, WM, WN, MODE, true, true><<<grid, 256, 0, st>>>(p);
  else if (vec) conv_igemm_kernel<BM, BN, WM, WN, MODE, true, false><<<grid, 256, 0, st>>>(p);
  else conv_igemm_kernel<BM, BN, WM, WN, MODE, false, false><<<grid, 256, 0, st>>>(p);
}

template <int MODE>
static int launch_igemm(GemmConvParams& p, bool vec, bool vec16, int splits, int cfg,
                        hipStream_t st) {
  if (MODE == MODE_WGRAD) vec16 = false;
  switch (cfg) {
    case 0: launch_cfg<MODE, 256, 32, 4, 1>(p, vec, vec16, splits, st); break;
    case 1: launch_cfg<MODE, 128, 64, 2, 2>(p, vec, vec16, splits, st); break;
    case 2: launch_cfg<MODE, 128, 96, 4, 1>(p, vec, vec16, splits, st); break;
    case 3: launch_cfg<MODE, 128, 128, 2, 2>(p, vec, vec16, splits, st); break;
    case 4: launch_cfg<MODE, 128, 160, 4, 1>(p, vec, vec16, splits, st); break;
    case 5: launch_cfg<MODE, 128, 192, 4, 1>(p, vec, vec16, splits, st); break;
    case 6: launch_cfg<MODE, 128, 224, 4, 1>(p, vec, vec16, splits, st); break;
    case 7: launch_cfg<MODE, 256, 64, 4, 1>(p, vec, vec16, splits, st); break;
    default: launch_cfg<MODE, 256, 128, 2, 2>(p, vec, vec16, splits, st); break;
  }
  return check_launch("conv_igemm_kernel");
}

static int fill_geom(const pld_conv_args* a, GemmConvParams& p) {
  PLD_CHECK_ARG(a && a->x1, "conv: null args/x1");
  PLD_CHECK_ARG(a->c1 > 0 && a->c2 >= 0 && (a->c2 == 0 || a->x2), "conv: bad channels");
  PLD_CHECK_ARG(a->n > 0 && a->h > 0 && a->w > 0 && a->kh > 0 && a->kw > 0 && a->sh > 0 &&
                    a->sw > 0 && a->oh > 0 && a->ow > 0 && a->cout > 0,
                "conv: bad geometry");
  PLD_CHECK_ARG((long)a->n * a->h * a->w * (a->c1 + a->c2) < (1L << 31) &&
                    (long)a->n * a->oh * a->ow * a->cout < (1L << 31),
                "conv: tensor too large for 32-bit indexing");
  p = GemmConvParams{};
  p.x1 = a->x1;
  p.x2 = a->x2;
  p.c1 = a->c1;
  p.c2 = a->c2;
  p.C = a->c1 + a->c2;
  p.n = a->n; p.h = a->h; p.w = a->w;
  p.kh = a->kh; p.kw = a->kw; p.sh = a->sh; p.sw = a->sw;
  p.pt = a->pad_t; p.pl = a->pad_l; p.oh = a->oh; p.ow = a->ow;
  p.in_scale = a->in_scale;
  p.in_shift = a->in_shift;
  p.in_act = a->in_act;
  p.dC = FastDiv((uint32_t)p.C);
  p.dKW = FastDiv((uint32_t)p.kw);
  p.dOW = FastDiv((uint32_t)p.ow);
  p.dOH = FastDiv((uint32_t)p.oh);
  p.dTaps = FastDiv((uint32_t)(p.kh * p.kw));
  return PLD_OK;
}


}  // namespace pld

using namespace pld;

// the direct, thin, wide, bf16x3 and BN helpers of the other files: conv_common.h, common.h

// a bf16x3 1x1 conv whose GEMM (fwd K = cin, N = cout; dgrad K = cout, N = cin) takes the wide
// kernel: unstrided single-source geometry that the exact thin kernel does not cover
static bool wide_conv(const pld_conv_args* a, int K, int N) {
  return a->math == PLD_MATH_BF16X3 && pld__thin_geom(a) && !pld__thin_ok(K, N) &&
         pld__wide_ok(K, N) && aligned16(a->x1);
}
constexpr int X3_BK = 32;
// bytes of a pre-split [N][K] filter (same size as fp32), 256-byte aligned
static size_t x3_split_bytes(long N, long K) { return ((size_t)N * K * 4 + 255) / 256 * 256; }

// bf16x3 eligibility: channel counts (vector staging); a fused input prologue on one source only
static bool x3_fwd_geom(int C, int c1, bool prologue, int taps) {
  return C % 8 == 0 && c1 % 8 == 0 && (!prologue || c1 == C) && taps <= 32;
}

// Schedule index space under PLD_MATH_BF16X3: [0, 2 n3) bf16x3 tiles (x split-K), [2 n3,
// 2 n3 + np) the bf16x3 patch kernel (3x3, 32-channel inputs; other shapes take the default
// tile), [2 n3 + np, 3 n3 + np) the bf16x3 tiles as a tile stream (conv_x3_kernel STREAM: a
// 1-D grid walking (tile, K-step) ranges), [3 n3 + np, 3 n3 + np + 3 nh) the row-band halo
// kernel (conv_x3_halo.hip: grid, split-K over whole chunks, tile stream), then the exact-fp32
// schedules — the
// per-shape autotuner may keep fp32 where it is faster (e.g. HBM-bound K <= 32 convs); it is
// never less accurate. Resolves (math, eligible geometry, tile) to (x3 kernel?, patch kernel?,
// stream?, halo?, tile in that space; halo: [0, 3 nh)).
static int x3_halo_base() { return 3 * pld__x3_num_cfg() + pld__x3_num_patch(); }
static int x3_sched_count() { return x3_halo_base() + 3 * pld__x3_num_halo(); }
static void resolve_sched(int math, bool geom_ok, int tile, bool& x3, int& t,
                          bool* patch = nullptr, bool* stream = nullptr, bool* halo = nullptr) {
  const int n3 = pld__x3_num_cfg(), np = pld__x3_num_patch(), nx = x3_sched_count();
  x3 = false;
  t = tile;
  if (patch) *patch = false;
  if (stream) *stream = false;
  if (halo) *halo = false;
  if (math != PLD_MATH_BF16X3) return;
  if (tile >= nx) {
    t = tile - nx;
    return;
  }
  if (!geom_ok) {
    t = -1;
    return;
  }
  x3 = true;
  if (tile >= x3_halo_base()) {  // halo schedule tile - base (callers that cannot: default)
    t = halo ? tile - x3_halo_base() : -1;
    if (halo) *halo = true;
  } else if (tile >= 2 * n3 + np) {  // tile stream of cfg tile - (2 n3 + np); callers that cannot
    t = stream ? tile - 2 * n3 - np : -1;  // run it take the default tile
    if (stream) *stream = true;
  } else if (tile >= 2 * n3) {
    t = patch ? tile - 2 * n3 : -1;
    if (patch) *patch = true;
  }
}
static bool x3_wgrad_geom(int c1, int c2, int cout, bool prologue) {
  return c1 % 16 == 0 && c2 % 16 == 0 && cout % 16 == 0 && !prologue;
}

// the x3 analogue of choose_tile (same cost model; WGRAD takes power-of-two tiles only)
static int x3_choose(long M, long N, long K, int requested, bool wgrad) {
  const int n = pld__x3_num_cfg();
  if (requested >= 0 && requested < 2 * n &&
      (!wgrad || pld__x3_wgrad_cfg_ok(requested % n)))
    return requested % n;
  int best = -1;
  double best_t = 1e300;
  for (int i = 0; i < n; ++i) {
    if (wgrad && !pld__x3_wgrad_cfg_ok(i)) continue;
    int bm, bn, tm, tn, occ;
    pld__x3_cfg_dims(i, &bm, &bn, &tm, &tn, &occ);
    const long blocks = (long)cdiv(M, bm) * cdiv(N, bn);
    const int per_wave = tm * tn;
    const double eff = per_wave >= 4 ? 1.0 : (per_wave == 3 ? 0.9 : (per_wave == 2 ? 0.8 : 0.55));
    const double rounds = std::ceil((double)blocks / (256.0 * occ));
    const double t_est = rounds * occ * (double)bm * bn * (double)K / eff;
    if (best < 0 || t_est < best_t * 0.97) {
      best_t = t_est;
      best = i;
    }
  }
  return best;
}

// K-step order of a bf16x3 FWD/DGRAD GEMM (GemmConvParams::kc_tap): tap-inner when a tap spans
// several 32-channel chunks (im2col re-reads then land in L2 one step apart instead of C/32 steps)
static int x3_kc_tap(int taps, int c1, int c2) {
  static const int mode = [] {
    const char* e = std::getenv("PLD_X3_TAP_INNER");
    return e ? std::atoi(e) : 1;
  }();
  return (mode && taps > 1 && c1 + c2 >= 64) ? (int)(cdiv(c1, X3_BK) + cdiv(c2, X3_BK)) : 0;
}
static long x3_ktiles(int kc_tap, int taps, long K) {
  return kc_tap ? (long)kc_tap * taps : (K + X3_BK - 1) / X3_BK;
}

static void x3_fwd_plan(long M, long N, long K, long ktiles, int tile, int& cfg, int& splits,
                        int& kt_per) {
  cfg = x3_choose(M, N, K, tile, false);
  const bool allow = tile >= pld__x3_num_cfg();
  int bm, bn, tm, tn, occ;
  pld__x3_cfg_dims(cfg, &bm, &bn, &tm, &tn, &occ);
  const long blocks = (long)cdiv(M, bm) * cdiv(N, bn);
  long s = 1;
  if (allow) {
    s = std::max<long>(1, (512 + blocks - 1) / blocks);
    s = std::min<long>(s, std::max<long>(1, ktiles / 8));
    s = std::min<long>(s, 16);
  }
  kt_per = (int)((ktiles + s - 1) / s);
  splits = (int)((ktiles + kt_per - 1) / kt_per);
}

// halo plan (h in [0, 3 nh): cfg h % nh; nh <= h < 2 nh: split-K over whole chunks, enough
// workgroups for two rounds of the 256 CUs (one resident each), >= 4 chunks per split; h >= 2 nh:
// the tile stream, planned by pld__x3_halo_stream_plan (splits = 1 here)
static void x3_halo_plan(long M, long N, int kc_tap, int h, int& cfg, int& splits,
                         int& kt_per) {
  const int nh = pld__x3_num_halo();
  cfg = h % nh;
  int bm, bn, tm, tn;
  pld__x3_halo_dims(cfg, &bm, &bn, &tm, &tn);
  const long blocks = (long)cdiv(M, bm) * cdiv(N, bn);
  long s = 1;
  if (h >= nh && h < 2 * nh) {
    s = std::max<long>(1, (512 + blocks - 1) / blocks);
    s = std::min<long>(s, std::max<long>(1, kc_tap / 4));
    s = std::min<long>(s, 16);
  }
  const long per = (kc_tap + s - 1) / s;  // chunks per split
  kt_per = (int)(per * 9);
  splits = (int)((kc_tap + per - 1) / per);
}
static bool x3_halo_is_stream(int h) { return h >= 2 * pld__x3_num_halo(); }

// tile-stream plan: T tiles of nk K-steps on occ resident workgroups per CU. As many tiles as
// resident slots or more: whole tiles per workgroup, balanced (the pipeline runs on from tile to
// tile); fewer: the (tile, K-step) space cut evenly over the slots, >= 16 K-steps each
// (stream-K: cut tiles are summed by the fixup kernel). Returns the grid; sets p.sk_*.
// (Round 5 measured cutting evenly also when whole tiles quantise badly — T / slots = 4.2 runs 5
// rounds — on the decoder dgrads: no faster than the grid, profiles/r05_stream_sweep.txt.)
static int x3_stream_plan(GemmConvParams& p, int cfg, long ktiles) {
  int bm, bn, tm, tn, occ;
  pld__x3_cfg_dims(cfg, &bm, &bn, &tm, &tn, &occ);
  const long tiles = (long)cdiv(p.M, bm) * cdiv(p.N, bn);
  const long slots = 256L * occ;
  p.sk_nk = (int)ktiles;
  p.sk_tiles = (int)tiles;
  p.sk_nnb = (int)cdiv(p.N, bn);
  long G;
  if (tiles >= slots) {
    const long per = cdiv(tiles, slots);
    G = cdiv(tiles, per);
    p.sk_align = 1;
  } else {
    G = std::min<long>(slots, std::max<long>(tiles, tiles * ktiles / 16));
    p.sk_align = (G == tiles) ? 1 : 0;
  }
  return (int)G;
}
static size_t x3_stream_slab_bytes(const GemmConvParams& p, int cfg, int G) {
  if (p.sk_align) return 0;
  int bm, bn, tm, tn, occ;
  pld__x3_cfg_dims(cfg, &bm, &bn, &tm, &tn, &occ);
  return sizeof(float) * 2 * (size_t)G * bm * bn;
}

// split-K plan for a forward / dgrad GEMM under schedule `tile`: enough workgroups for ~3 per
// CU, >= 16 K-steps each; the split-K schedules (tile >= kNumCfg) only
static void fwd_split_plan(long M, long N, long K, int tile, int& cfg, int& splits,
                           int& kt_per) {
  cfg = choose_tile(M, N, K, 1, tile);
  const bool allow = tile >= kNumCfg;
  const long ktiles = (K + BK - 1) / BK;
  const long blocks = (long)cdiv(M, kTiles[cfg].bm) * cdiv(N, kTiles[cfg].bn);
  long s = 1;
  if (allow) {
    s = std::max<long>(1, (768 + blocks - 1) / blocks);
    s = std::min<long>(s, std::max<long>(1, ktiles / 16));
    s = std::min<long>(s, 16);
  }
  kt_per = (int)((ktiles + s - 1) / s);
  splits = (int)((ktiles + kt_per - 1) / kt_per);
}

// bytes one workgroup's A operand can span from its base image (buffer offsets are 32-bit)
static long fwd_span_bytes(const GemmConvParams& p, int bm) {
  const long imgs = bm / ((long)p.oh * p.ow) + 2;
  return imgs * p.h * p.w * (long)std::max(p.c1, p.c2) * 4;
}

// pld_conv2d_fwd_bn_stats -> run_fwd_gemm: where the forward GEMM runs unsplit on a tile
// kernel (bf16x3 im2col or exact fp32), its epilogue writes the BN statistics partials into
// `buf` and `parts` reports their count (0: not fused, the caller takes the separate pass)
struct FwdStatsReq {
  double* buf = nullptr;
  int parts = 0;
};
static thread_local FwdStatsReq g_fwd_stats;

static void fwd_stats_attach(GemmConvParams& p, int bm, int tm) {
  if (!g_fwd_stats.buf || p.acc1 || p.split < p.N) return;
  p.stats = g_fwd_stats.buf;
  p.stats_parts = (int)cdiv(p.M, bm) * (bm / (32 * tm));
  g_fwd_stats.parts = p.stats_parts;
}

static int run_fwd_gemm(GemmConvParams& p, bool vec, bool vec16, int tile, void* ws,
                        size_t ws_bytes, hipStream_t st, const char* who, int math = 0) {
  int cfg, splits, kt_per;
  bool x3;
  bool patch, stream, halo;
  resolve_sched(math, x3_fwd_geom(p.C, p.c1, p.in_scale != nullptr, p.kh * p.kw), tile, x3,
                tile, &patch, &stream, &halo);
  if (halo && (!pld__x3_halo_ok(&p) || p.w > pld__x3_halo_wmax(tile % pld__x3_num_halo()))) {
    // halo schedule on another shape (or a map wider than it takes): default tile
    halo = false;
    tile = -1;
  }
  const long in_bytes = (long)p.n * p.h * p.w * std::max(p.c1, p.c2) * 4;
  if (stream && (p.in_scale || in_bytes >= MAX_RECORDS)) {  // stream: no prologue, whole-tensor
    stream = false;                                         // descriptors
    tile = -1;
  }
  if (patch && !pld__x3_patch_ok(&p, tile)) {  // patch schedule on another shape: default tile
    patch = false;
    tile = -1;
  }
  if (x3) {
    PLD_CHECK_ARG(aligned16(p.x1) && (!p.x2 || aligned16(p.x2)) && aligned16(p.bmat) &&
                      (!p.bsplit || aligned16(p.bsplit)) &&
                      (!p.in_scale || (aligned16(p.in_scale) && aligned16(p.in_shift))),
                  "%s: bf16x3 operands must be 16-byte aligned", who);
    if (!p.bsplit) {  // the kernel stages a pre-split filter: split into the workspace's tail
      const size_t sb = x3_split_bytes(p.N, p.K);
      PLD_CHECK_ARG(ws && ws_bytes >= sb, "%s: workspace %zu < %zu bytes (filter split)", who,
                    ws_bytes, sb);
      ws_bytes -= sb;
      float* wsp = (float*)((char*)ws + ws_bytes);
      int rc = pld_filter_split(p.bmat, p.N, p.K, wsp, st);
      if (rc) return rc;
      p.bsplit = wsp;
    }
    if (patch) return pld__x3_patch_launch(&p, tile, st);
    if (halo) {
      p.kc1 = (int)cdiv(p.c1, X3_BK);
      p.kc_tap = p.kc1 + (int)cdiv(p.c2, X3_BK);
      x3_halo_plan(p.M, p.N, p.kc_tap, tile, cfg, splits, kt_per);
      if (splits == 1) {
        p.ktiles_per_split = 0;
        p.zstride = 0;
        int bm, bn, tm, tn;
        pld__x3_halo_dims(cfg, &bm, &bn, &tm, &tn);
        int G = 0;
        if (x3_halo_is_stream(tile)) {
          G = pld__x3_halo_stream_plan(&p, cfg);
          const size_t need = pld__x3_halo_stream_slab_bytes(cfg, G, p.sk_align);
          PLD_CHECK_ARG(need == 0 || (ws && ws_bytes >= need),
                        "%s: halo tile-stream workspace %zu < %zu bytes", who, ws_bytes, need);
          p.sk_slab = need ? (float*)ws : nullptr;
        }
        fwd_stats_attach(p, bm, tm);
        return pld__x3_halo_launch(&p, cfg, 1, G, st);
      }
      const size_t need = sizeof(float) * (size_t)splits * p.M * p.N;
      PLD_CHECK_ARG(ws && ws_bytes >= need, "%s: split-K workspace %zu < %zu bytes", who,
                    ws_bytes, need);
      GemmConvParams q = p;
      q.ktiles_per_split = kt_per;
      q.zstride = (long)p.M * p.N;
      q.out1 = (float*)ws;
      int rc = pld__x3_halo_launch(&q, cfg, splits, 0, st);
      if (rc) return rc;
      const long n = (long)p.M * p.N;
      splitk_out_kernel<<<std::min<unsigned>(cdiv(n, 256), 8192), 256, 0, st>>>(
          (const float*)ws, splits, p.M, p.N, p.bias, p.out1, p.ld1, p.acc1, p.out2, p.ld2,
          p.acc2, p.split);
      return check_launch("splitk_out_kernel");
    }
    p.kc_tap = x3_kc_tap(p.kh * p.kw, p.c1, p.c2);
    p.kc1 = (int)cdiv(p.c1, X3_BK);
    if (stream) {
      cfg = tile;
      const int G = x3_stream_plan(p, cfg, x3_ktiles(p.kc_tap, p.kh * p.kw, p.K));
      const size_t need = x3_stream_slab_bytes(p, cfg, G);
      PLD_CHECK_ARG(need == 0 || (ws && ws_bytes >= need),
                    "%s: tile-stream workspace %zu < %zu bytes", who, ws_bytes, need);
      PLD_CHECK_ARG((long)p.N * p.K * 4 < MAX_RECORDS, "%s: filter too large", who);
      p.sk_slab = need ? (float*)ws : nullptr;
      p.ktiles_per_split = 0;
      p.zstride = 0;
      int bm, bn, tm, tn, occ;
      pld__x3_cfg_dims(cfg, &bm, &bn, &tm, &tn, &occ);
      fwd_stats_attach(p, bm, tm);
      return pld__x3_launch(&p, MODE_FWD, 1, cfg, G, st);
    }
    x3_fwd_plan(p.M, p.N, p.K, x3_ktiles(p.kc_tap, p.kh * p.kw, p.K), tile, cfg, splits, kt_per);
    int bm, bn, tm, tn, occ;
    pld__x3_cfg_dims(cfg, &bm, &bn, &tm, &tn, &occ);
    PLD_CHECK_ARG(fwd_span_bytes(p, bm) < MAX_RECORDS && (long)p.N * p.K * 4 < MAX_RECORDS,
                  "%s: image or filter too large for 32-bit buffer offsets", who);
  } else {
    fwd_split_plan(p.M, p.N, p.K, tile, cfg, splits, kt_per);
  }
  auto launch = [&](GemmConvParams& q, int sp) {
    return x3 ? pld__x3_launch(&q, MODE_FWD, sp, cfg, 0, st)
              : launch_igemm<MODE_FWD>(q, vec, vec16, sp, cfg, st);
  };
  if (x3) {
    if (splits == 1) {
      p.ktiles_per_split = 0;
      p.zstride = 0;
      int bm, bn, tm, tn, occ;
      pld__x3_cfg_dims(cfg, &bm, &bn, &tm, &tn, &occ);
      fwd_stats_attach(p, bm, tm);
      return launch(p, 1);
    }
  } else {
  PLD_CHECK_ARG(fwd_span_bytes(p, kTiles[cfg].bm) < MAX_RECORDS &&
                    (long)p.N * p.K * 4 < MAX_RECORDS,
                "%s: image or filter too large for 32-bit buffer offsets", who);
  if (splits == 1) {
    p.ktiles_per_split = 0;
    p.zstride = 0;
    // rows per wave of the exact-fp32 tiles (launch_igemm's WM: BM / WM = 64 for cfg 1,
    // which kTiles' cost-model tm does not state)
    static const int kWaveRows[kNumCfg] = {64, 64, 32, 64, 32, 32, 32, 64, 128};
    fwd_stats_attach(p, kTiles[cfg].bm, kWaveRows[cfg] / 32);
    return launch_igemm<MODE_FWD>(p, vec, vec16, 1, cfg, st);
  }
  }
  const size_t need = sizeof(float) * (size_t)splits * p.M * p.N;
  PLD_CHECK_ARG(ws && ws_bytes >= need, "%s: split-K workspace %zu < %zu bytes", who, ws_bytes,
                need);
  GemmConvParams q = p;
  q.ktiles_per_split = kt_per;
  q.zstride = (long)p.M * p.N;
  q.out1 = (float*)ws;
  int rc = launch(q, splits);
  if (rc) return rc;
  const long n = (long)p.M * p.N;
  splitk_out_kernel<<<std::min<unsigned>(cdiv(n, 256), 8192), 256, 0, st>>>(
      (const float*)ws, splits, p.M, p.N, p.bias, p.out1, p.ld1, p.acc1, p.out2, p.ld2, p.acc2,
      p.split);
  return check_launch("splitk_out_kernel");
}

static size_t fwd_ws_bytes(long M, long N, long K, int taps, int c1, int c2, int tile,
                           int math = 0, bool geom = false, bool have_split = true) {
  int cfg, splits, kt_per;
  bool x3, stream, halo;
  resolve_sched(math, geom, tile, x3, tile, nullptr, &stream, &halo);
  size_t b;
  if (halo) {  // (a shape the halo kernel does not take runs the default tile: no workspace)
    const int kc = (int)(cdiv(c1, X3_BK) + cdiv(c2, X3_BK));
    x3_halo_plan(M, N, kc, tile, cfg, splits, kt_per);
    b = splits > 1 ? sizeof(float) * (size_t)splits * M * N : 0;
    if (x3_halo_is_stream(tile)) {
      GemmConvParams q{};
      q.M = (int)M;
      q.N = (int)N;
      q.kc_tap = kc;
      const int G = pld__x3_halo_stream_plan(&q, cfg);
      b = pld__x3_halo_stream_slab_bytes(cfg, G, q.sk_align);
    }
  } else if (stream) {  // (an input prologue runs on the default tile: no workspace either way)
    GemmConvParams q{};
    q.M = (int)M;
    q.N = (int)N;
    const int G = x3_stream_plan(q, tile, x3_ktiles(x3_kc_tap(taps, c1, c2), taps, K));
    b = x3_stream_slab_bytes(q, tile, G);
  } else {
    if (x3)
      x3_fwd_plan(M, N, K, x3_ktiles(x3_kc_tap(taps, c1, c2), taps, K), tile, cfg, splits,
                  kt_per);
    else fwd_split_plan(M, N, K, tile, cfg, splits, kt_per);
    b = splits > 1 ? sizeof(float) * (size_t)splits * M * N : 0;
  }
  if (x3 && !have_split) b = (b + 255) / 256 * 256 + x3_split_bytes(N, K);
  return b;
}

extern "C" int pld_filter_to_native(const float* w_hwio, int kh, int kw, int cin, int cout,
                                    float* w_ohwi, void* stream) {
  PLD_CHECK_ARG(w_hwio && w_ohwi && kh > 0 && kw > 0 && cin > 0 && cout > 0,
                "pld_filter_to_native: bad args");
  const long n = (long)kh * kw * cin * cout;
  filter_native_kernel<<<std::min<unsigned>(cdiv(n, 256), 4096), 256, 0, as_stream(stream)>>>(
      w_hwio, kh * kw, cin, cout, w_ohwi);
  return check_launch("filter_native_kernel");
}

extern "C" int pld_filter_to_dgrad(const float* w_hwio, int kh, int kw, int cin, int cout,
                                   float* w_dgrad, void* stream) {
  PLD_CHECK_ARG(w_hwio && w_dgrad && kh > 0 && kw > 0 && cin > 0 && cout > 0,
                "pld_filter_to_dgrad: bad args");
  const long n = (long)kh * kw * cin * cout;
  filter_dgrad_kernel<<<std::min<unsigned>(cdiv(n, 256), 4096), 256, 0, as_stream(stream)>>>(
      w_hwio, kh, kw, cin, cout, w_dgrad);
  return check_launch("filter_dgrad_kernel");
}

extern "C" int pld_filter_refresh(const float* w_hwio, int kh, int kw, int cin, int cout,
                                  float* w_ohwi, void* w_ohwi_split, float* w_dgrad,
                                  void* w_dgrad_split, void* stream) {
  PLD_CHECK_ARG(w_hwio && w_ohwi && kh > 0 && kw > 0 && cin > 0 && cout > 0,
                "pld_filter_refresh: bad args");
  PLD_CHECK_ARG(!w_dgrad_split || w_dgrad, "pld_filter_refresh: dgrad split without dgrad");
  hipStream_t st = as_stream(stream);
  const int taps = kh * kw;
  const long R = (long)taps * cin;
  int rc;
  if (R % 8 == 0 && aligned16(w_ohwi) && (!w_ohwi_split || aligned16(w_ohwi_split)) &&
      R < (1L << 30)) {
    const dim3 grid((unsigned)cdiv(R, 64), (unsigned)cdiv(cout, 64));
    filter_native_tiled_kernel<<<grid, 256, 0, st>>>(w_hwio, (int)R, cout, w_ohwi,
                                                     (u32x4r*)w_ohwi_split);
    rc = check_launch("filter_native_tiled_kernel");
  } else {
    rc = pld_filter_to_native(w_hwio, kh, kw, cin, cout, w_ohwi, stream);
    if (!rc && w_ohwi_split) rc = pld_filter_split(w_ohwi, cout, (int)R, w_ohwi_split, stream);
  }
  if (rc || !w_dgrad) return rc;
  const long n = (long)cin * taps * cout;
  if (cout % 8 == 0 && aligned16(w_hwio) && aligned16(w_dgrad) &&
      (!w_dgrad_split || aligned16(w_dgrad_split))) {
    filter_dgrad_rows_kernel<<<std::min<unsigned>(cdiv(n / 8, 256), 8192), 256, 0, st>>>(
        w_hwio, taps, cin, cout, w_dgrad, (u32x4r*)w_dgrad_split);
    return check_launch("filter_dgrad_rows_kernel");
  }
  rc = pld_filter_to_dgrad(w_hwio, kh, kw, cin, cout, w_dgrad, stream);
  if (!rc && w_dgrad_split)
    rc = pld_filter_split(w_dgrad, cin, taps * cout, w_dgrad_split, stream);
  return rc;
}

extern "C" int pld_filter_refresh_plan(int kh, int kw, int cin, int cout, const void* w_hwio,
                                       const void* w_ohwi, const void* w_ohwi_split,
                                       const void* w_dgrad, const void* w_dgrad_split) {
  if (!w_hwio || !w_ohwi || kh <= 0 || kw <= 0 || cin <= 0 || cout <= 0) return 0;
  if (w_dgrad_split && !w_dgrad) return 0;
  const long R = (long)kh * kw * cin;
  if (R % 8 || R >= (1L << 30) || !aligned16(w_ohwi) || (w_ohwi_split && !aligned16(w_ohwi_split)))
    return 0;
  long nblk = cdiv(R, 64) * cdiv(cout, 64);
  if (w_dgrad) {
    if (cout % 8 || !aligned16(w_hwio) || !aligned16(w_dgrad) ||
        (w_dgrad_split && !aligned16(w_dgrad_split)))
      return 0;
    nblk += refresh_dgrad_blocks(R * cout / 8);
  }
  return nblk < (1L << 30) ? (int)nblk : 0;
}

extern "C" int pld_filter_refresh_multi(const pld_filter_refresh_desc* table_dev, int count,
                                        int total_blocks, void* stream) {
  PLD_CHECK_ARG(table_dev && count > 0 && total_blocks > 0, "pld_filter_refresh_multi: bad args");
  filter_refresh_multi_kernel<<<total_blocks, 256, 0, as_stream(stream)>>>(table_dev, count);
  return check_launch("filter_refresh_multi_kernel");
}

extern "C" int pld_conv2d_fwd(const pld_conv_args* a, const float* w_ohwi, const float* bias,
                              float* y, int accumulate, void* stream) {
  GemmConvParams p;
  int rc = fill_geom(a, p);
  if (rc) return rc;
  PLD_CHECK_ARG(w_ohwi && y, "pld_conv2d_fwd: null w/y");
  if (pld__stem3x3_eligible(a) && aligned16(y))
    return pld__stem3x3_fwd(a, w_ohwi, bias, y, accumulate, nullptr, stream);
  if (pld__scalar1x1_eligible(a) && aligned16(a->x1) && aligned16(y))
    return pld__scalar1x1_apply(a->x1, w_ohwi, bias, y, (long)a->n * a->h * a->w, accumulate,
                                stream);
  if (pld__skinny_eligible(a) && aligned16(a->x1))
    return pld__skinny_fwd(a, w_ohwi, bias, y, accumulate, stream);
  if (pld__thin_geom(a) && pld__thin_ok(a->c1, a->cout) && aligned16(a->x1) && aligned16(y) &&
      aligned16(w_ohwi))
    return pld__thin_gemm(a->x1, w_ohwi, bias, y, (long)a->n * a->h * a->w, a->c1, a->cout,
                          accumulate, stream, nullptr);
  if (wide_conv(a, a->c1, a->cout) && aligned16(w_ohwi) && aligned16(y))
    return pld__wide_gemm(a->x1, w_ohwi, bias, y, (long)a->n * a->h * a->w, a->c1, a->cout,
                          accumulate, stream, nullptr);
  p.bmat = w_ohwi;
  p.bsplit = (const float*)a->w_split;
  p.M = a->n * a->oh * a->ow;
  p.N = a->cout;
  p.K = a->kh * a->kw * p.C;
  p.bias = bias;
  p.out1 = y;
  p.ld1 = a->cout;
  p.acc1 = accumulate;
  p.split = a->cout;
  const bool vec = (p.c1 % 4 == 0) && (p.c2 % 4 == 0) && aligned16(p.x1) &&
                   (!p.x2 || aligned16(p.x2)) && aligned16(w_ohwi) &&
                   (!p.in_scale || (aligned16(p.in_scale) && aligned16(p.in_shift)));
  const bool vec16 = vec && (p.c1 % 16 == 0) && (p.c2 % 16 == 0);
  return run_fwd_gemm(p, vec, vec16, a->tile, a->ws, a->ws_bytes, as_stream(stream),
                      "pld_conv2d_fwd", a->math);
}

// conv forward + the batch statistics of its output for the BatchNormalization that follows:
// where the kernel the conv runs on can gather them as it stores its tile (thin and wide 1x1),
// the output is not read back; otherwise pld_conv2d_fwd + pld_bn_stats.
static bool fwd_stats_thin(const pld_conv_args* a, const float* w_ohwi, const float* y) {
  return !pld__skinny_eligible(a) && pld__thin_geom(a) && pld__thin_ok(a->c1, a->cout) &&
         aligned16(a->x1) && aligned16(y) && aligned16(w_ohwi);
}
static bool fwd_stats_wide(const pld_conv_args* a, const float* w_ohwi, const float* y) {
  return !pld__skinny_eligible(a) && wide_conv(a, a->c1, a->cout) && aligned16(w_ohwi) &&
         aligned16(y);
}

extern "C" size_t pld_conv2d_fwd_bn_stats_workspace_size(const pld_conv_args* a) {
  if (!a || a->n <= 0 || a->oh <= 0 || a->ow <= 0 || a->cout <= 0) return 0;
  const long rows = (long)a->n * a->oh * a->ow;
  const size_t thin = sizeof(double) * 2 * (size_t)a->cout * pld__thin_stats_parts(rows);
  const size_t wide = pld__wide_ok(a->c1, a->cout)
                          ? sizeof(double) * 2 * (size_t)a->cout *
                                pld__wide_stats_parts(rows, a->c1, a->cout)
                          : 0;
  // GEMM epilogue partials: cdiv(M, BM) x BM / (32 TM) <= M / 32 + 8 per channel
  const size_t gemm = sizeof(double) * 2 * (size_t)a->cout * (cdiv(rows, 32) + 8);
  const size_t stem =
      pld__stem3x3_eligible(a) ? sizeof(double) * 2 * (size_t)a->cout * pld__stem3x3_parts(a) : 0;
  return std::max(std::max(std::max(std::max(thin, wide), gemm), stem),
                  pld_channel_reduce_workspace_size(rows, a->cout));
}

extern "C" int pld_conv2d_fwd_bn_stats(const pld_conv_args* a, const float* w_ohwi,
                                       const float* bias, float* y, float eps, float momentum,
                                       float* mean, float* invstd, float* moving_mean,
                                       float* moving_var, void* ws, size_t ws_bytes,
                                       void* stream) {
  PLD_CHECK_ARG(a && w_ohwi && y && mean && invstd && ws, "pld_conv2d_fwd_bn_stats: bad args");
  PLD_CHECK_ARG(ws_bytes >= pld_conv2d_fwd_bn_stats_workspace_size(a),
                "pld_conv2d_fwd_bn_stats: workspace too small");
  PLD_CHECK_ARG((moving_mean == nullptr) == (moving_var == nullptr),
                "pld_conv2d_fwd_bn_stats: moving_mean/moving_var must both be given or both NULL");
  const long rows = (long)a->n * a->oh * a->ow;
  if (pld__stem3x3_eligible(a) && aligned16(y)) {
    int rc = pld__stem3x3_fwd(a, w_ohwi, bias, y, 0, (double*)ws, stream);
    if (rc) return rc;
    return pld__bn_stats_finish((const double*)ws, pld__stem3x3_parts(a), rows, a->cout, eps,
                                momentum, mean, invstd, moving_mean, moving_var,
                                as_stream(stream));
  }
  if (fwd_stats_thin(a, w_ohwi, y)) {
    int rc = pld__thin_gemm(a->x1, w_ohwi, bias, y, rows, a->c1, a->cout, 0, stream,
                            (double*)ws);
    if (rc) return rc;
    return pld__bn_stats_finish((const double*)ws, pld__thin_stats_parts(rows), rows, a->cout,
                                eps, momentum, mean, invstd, moving_mean, moving_var,
                                as_stream(stream));
  }
  if (fwd_stats_wide(a, w_ohwi, y)) {
    int rc = pld__wide_gemm(a->x1, w_ohwi, bias, y, rows, a->c1, a->cout, 0, stream,
                            (double*)ws);
    if (rc) return rc;
    return pld__bn_stats_finish((const double*)ws, pld__wide_stats_parts(rows, a->c1, a->cout),
                                rows, a->cout, eps, momentum, mean, invstd, moving_mean,
                                moving_var, as_stream(stream));
  }
  g_fwd_stats = FwdStatsReq{(double*)ws, 0};
  int rc = pld_conv2d_fwd(a, w_ohwi, bias, y, 0, stream);
  const int parts = g_fwd_stats.parts;
  g_fwd_stats = FwdStatsReq{};
  if (rc) return rc;
  if (parts > 0)  // gathered by the GEMM epilogue
    return pld__bn_stats_finish((const double*)ws, parts, rows, a->cout, eps, momentum, mean,
                                invstd, moving_mean, moving_var, as_stream(stream));
  return pld_bn_stats(y, rows, a->cout, eps, momentum, mean, invstd, moving_mean, moving_var, ws,
                      stream);
}

extern "C" int pld_conv_num_tiles(void) { return kNumTiles; }

extern "C" int pld_conv_num_schedules(int math) {
  return math == PLD_MATH_BF16X3 ? x3_sched_count() + kNumTiles : kNumTiles;
}

extern "C" int pld_conv_schedule_class(int math, int idx) {
  if (idx < 0 || idx >= pld_conv_num_schedules(math)) return -1;
  const int nf = kNumTiles / 2;  // fp32: [tiles | tiles x split-K]
  if (math != PLD_MATH_BF16X3) return idx < nf ? PLD_SCHED_FP32 : PLD_SCHED_FP32_SPLIT;
  const int n3 = pld__x3_num_cfg(), np = pld__x3_num_patch(), nx = x3_sched_count();
  if (idx < n3) return PLD_SCHED_X3;
  if (idx < 2 * n3) return PLD_SCHED_X3_SPLIT;
  if (idx < 2 * n3 + np) return PLD_SCHED_X3_PATCH;
  if (idx < x3_halo_base()) return PLD_SCHED_X3_STREAM;
  if (idx < nx) return PLD_SCHED_X3_HALO;
  return idx - nx < nf ? PLD_SCHED_FP32 : PLD_SCHED_FP32_SPLIT;
}

extern "C" const char* pld_conv_schedule_desc(int math, int idx) {
  // one slot per schedule index and math, written once (the tables are constant)
  static char names[2][128][24];
  const int cls = pld_conv_schedule_class(math, idx);
  if (cls < 0 || idx >= 128) return nullptr;
  char* out = names[math == PLD_MATH_BF16X3 ? 1 : 0][idx];
  if (out[0]) return out;
  const int n3 = pld__x3_num_cfg(), np = pld__x3_num_patch();
  const int nx = math == PLD_MATH_BF16X3 ? x3_sched_count() : 0;
  int bm = 0, bn = 0, tm, tn, occ;
  switch (cls) {
    case PLD_SCHED_X3:
    case PLD_SCHED_X3_SPLIT:
      pld__x3_cfg_dims(idx % n3, &bm, &bn, &tm, &tn, &occ);
      snprintf(out, 24, "%s/%dx%d", cls == PLD_SCHED_X3 ? "x3" : "x3split", bm, bn);
      break;
    case PLD_SCHED_X3_STREAM:
      pld__x3_cfg_dims(idx - 2 * n3 - np, &bm, &bn, &tm, &tn, &occ);
      snprintf(out, 24, "x3stream/%dx%d", bm, bn);
      break;
    case PLD_SCHED_X3_PATCH:
      snprintf(out, 24, "x3patch/%d", pld__x3_patch_bn(idx - 2 * n3));
      break;
    case PLD_SCHED_X3_HALO: {
      const int h = idx - x3_halo_base(), nh = pld__x3_num_halo();
      pld__x3_halo_dims(h % nh, &bm, &bn, &tm, &tn);
      // two workgroups per CU: "x3halo28..." (maps up to 28 wide), "x3halo2..." (up to 56)
      const int wm = pld__x3_halo_wmax(h % nh), two = pld__x3_halo_occ2(h % nh);
      snprintf(out, 24, "x3halo%s%s/%dx%d", wm == 28 ? "28" : two ? "2" : "",
               h < nh ? "" : h < 2 * nh ? "split" : "stream", bm, bn);
      break;
    }
    default: {
      const TileCfg& t = kTiles[(idx - nx) % kNumCfg];
      snprintf(out, 24, "%s/%dx%d", cls == PLD_SCHED_FP32 ? "fp32" : "fp32split", t.bm, t.bn);
    }
  }
  return out;
}

extern "C" int pld_conv_kernel_kind(const pld_conv_args* a, int mode) {
  if (!a || mode < 0 || mode > 2) return -1;
  if (mode == 0 && pld__stem3x3_eligible(a)) return PLD_KIND_DIRECT;
  if (pld__scalar1x1_eligible(a)) return PLD_KIND_DIRECT;
  if (pld__skinny_eligible(a) && !(mode == 1 && (a->sh != 1 || a->sw != 1)))
    return PLD_KIND_DIRECT;
  if (mode != 2 && pld__thin_geom(a) &&
      (mode == 0 ? pld__thin_ok(a->c1, a->cout) : pld__thin_ok(a->cout, a->c1)))
    return PLD_KIND_DIRECT;
  if (mode != 2 && (mode == 0 ? wide_conv(a, a->c1, a->cout) : wide_conv(a, a->cout, a->c1)))
    return PLD_KIND_DIRECT;
  bool geom, x3;
  int t;
  if (mode == 2)
    geom = x3_wgrad_geom(a->c1, a->c2, a->cout, a->in_scale != nullptr);
  else if (mode == 1)
    geom = x3_fwd_geom(a->cout, a->cout, false, a->kh * a->kw);
  else
    geom = x3_fwd_geom(a->c1 + a->c2, a->c1, a->in_scale != nullptr, a->kh * a->kw);
  resolve_sched(a->math, geom, a->tile, x3, t);
  return x3 ? PLD_KIND_BF16X3 : PLD_KIND_FP32;
}

// the name of the main kernel a conv call launches (for per-kernel roofline accounting and for
// matching HIP-event timings with rocprof's kernel names); "" on bad arguments. Split-K slab
// reductions a call may add are not named (they are part of the call's time).
static bool wgrad_patch_geom(const pld_conv_args* a);
extern "C" const char* pld_conv_kernel_name(const pld_conv_args* a, int mode) {
  const int kind = pld_conv_kernel_kind(a, mode);
  if (kind < 0) return "";
  if (kind == PLD_KIND_DIRECT) {
    if (mode == 0 && pld__stem3x3_eligible(a)) return "stem3x3_kernel";
    if (pld__scalar1x1_eligible(a))
      return mode == 2 ? "scalar1x1_wgrad_kernel" : "scalar1x1_kernel";
    if (pld__skinny_eligible(a))
      return mode == 0 ? "skinny_fwd_kernel" : mode == 1 ? "skinny_dgrad_kernel"
                                                         : "skinny_wgrad_kernel";
    if (mode == 0 ? wide_conv(a, a->c1, a->cout) : wide_conv(a, a->cout, a->c1))
      return "wide1x1_kernel";
    return "thin1x1_kernel";
  }
  if (kind == PLD_KIND_FP32) return "conv_igemm_kernel";
  if (mode != 2 && pld_conv_schedule_class(a->math, a->tile) == PLD_SCHED_X3_HALO) {
    // FWD view (dgrad: the input is dY, cout channels, one source): pld__x3_halo_ok's geometry
    const int c1 = mode == 0 ? a->c1 : a->cout, c2 = mode == 0 ? a->c2 : 0;
    const int w = mode == 0 ? a->w : a->ow, h = mode == 0 ? a->h : a->oh;
    const int ow = mode == 0 ? a->ow : a->w, oh = mode == 0 ? a->oh : a->h;
    const int wmax = pld__x3_halo_wmax((a->tile - x3_halo_base()) % pld__x3_num_halo());
    const bool ok = a->kh == 3 && a->kw == 3 && a->sh == 1 && a->sw == 1 && a->in_scale == nullptr &&
                    oh == h && ow == w && w <= wmax && c1 % 8 == 0 && c2 % 8 == 0 &&
                    a->pad_t >= 0 && a->pad_t <= 2 && a->pad_l >= 0 && a->pad_l <= 2;
    return ok ? "conv_x3_halo_kernel" : "conv_x3_kernel";
  }
  if (pld_conv_schedule_class(a->math, a->tile) != PLD_SCHED_X3_PATCH) return "conv_x3_kernel";
  const int cfg = a->tile - 2 * pld__x3_num_cfg();
  if (mode == 2)
    return wgrad_patch_geom(a) ? (pld__x3_patch_wgrad_cw(a->cout) == 64
                                      ? "conv_x3_patch_wgrad64_pc_kernel"
                                      : "conv_x3_patch_wgrad_pc_kernel")
                               : "conv_x3_kernel";
  // FWD view (dgrad: the input is dY, cout channels, one source)
  const int c1 = mode == 0 ? a->c1 : a->cout, c2 = mode == 0 ? a->c2 : 0;
  const bool geo = a->kh == 3 && a->kw == 3 && a->sh == 1 && a->sw == 1 &&
                   a->in_scale == nullptr && a->pad_t >= 0 && a->pad_t <= 2 && a->pad_l >= 0 &&
                   a->pad_l <= 2;
  if (!geo) return "conv_x3_kernel";
  if (c1 == 32 && c2 == 0) return "conv_x3_patch_kernel";
  return (cfg == 0 && c1 % 16 == 0 && c2 % 16 == 0) ? "conv_x3_patch_mc_pc_kernel"
                                                      : "conv_x3_kernel";
}

extern "C" size_t pld_conv2d_fwd_workspace_size(const pld_conv_args* a) {
  if (!a || a->n <= 0 || a->c1 <= 0 || a->cout <= 0 || a->oh <= 0 || a->ow <= 0) return 0;
  if (pld__skinny_eligible(a) || pld__scalar1x1_eligible(a) || pld__stem3x3_eligible(a)) return 0;
  return fwd_ws_bytes((long)a->n * a->oh * a->ow, a->cout,
                      (long)a->kh * a->kw * (a->c1 + a->c2), a->kh * a->kw, a->c1, a->c2, a->tile,
                      a->math,
                      x3_fwd_geom(a->c1 + a->c2, a->c1, a->in_scale != nullptr, a->kh * a->kw),
                      a->w_split != nullptr);
}

static size_t strided_tmp_bytes(const pld_conv_args* a) {
  return ((sizeof(float) * (size_t)a->n * a->oh * a->ow * (a->c1 + a->c2)) + 255) / 256 * 256;
}

extern "C" size_t pld_conv2d_dgrad_workspace_size(const pld_conv_args* a) {
  if (!a || a->n <= 0 || a->c1 <= 0 || a->cout <= 0 || a->h <= 0 || a->w <= 0) return 0;
  if (pld__skinny_eligible(a) || pld__scalar1x1_eligible(a)) return 0;
  const bool geom = x3_fwd_geom(a->cout, a->cout, false, a->kh * a->kw);
  const bool hs = a->w_split != nullptr;
  if (a->sh != 1 || a->sw != 1)  // 1x1 strided: GEMM into a compact tmp, then scatter
    return strided_tmp_bytes(a) + fwd_ws_bytes((long)a->n * a->oh * a->ow, a->c1 + a->c2,
                                               a->cout, 1, a->cout, 0, a->tile, a->math, geom,
                                               hs);
  return fwd_ws_bytes((long)a->n * a->h * a->w, a->c1 + a->c2, (long)a->kh * a->kw * a->cout,
                      a->kh * a->kw, a->cout, 0, a->tile, a->math, geom, hs);
}

extern "C" int pld_conv2d_dgrad(const pld_conv_args* a, const float* dy, const float* w_dgrad,
                                float* dx1, int accumulate1, float* dx2, int accumulate2,
                                void* stream) {
  PLD_CHECK_ARG(a && dy && w_dgrad && dx1, "pld_conv2d_dgrad: null pointer");
  PLD_CHECK_ARG(a->c2 == 0 || dx2, "pld_conv2d_dgrad: dx2 required for a two-source conv");
  PLD_CHECK_ARG(a->in_scale == nullptr,
                "pld_conv2d_dgrad: the input prologue's gradient is the caller's (pass NULL)");
  if (a->sh != 1 || a->sw != 1) {
    // ResNet projection / downsampling convs (1x1, stride s, no padding): a plain GEMM
    // t[img][oy][ox][:] = dy[img][oy][ox][:] . W^T, scattered to the stride grid
    PLD_CHECK_ARG(a->kh == 1 && a->kw == 1 && a->pad_t == 0 && a->pad_l == 0 && a->sh > 0 &&
                      a->sw > 0,
                  "pld_conv2d_dgrad: strided dgrad is implemented for 1x1 unpadded convs only");
    PLD_CHECK_ARG(a->n > 0 && a->oh > 0 && a->ow > 0 && a->h > 0 && a->w > 0 && a->cout > 0,
                  "pld_conv2d_dgrad: bad geometry");
    const size_t tb = strided_tmp_bytes(a);
    const size_t need = pld_conv2d_dgrad_workspace_size(a);
    PLD_CHECK_ARG(a->ws && a->ws_bytes >= need, "pld_conv2d_dgrad: strided workspace %zu < %zu",
                  a->ws_bytes, need);
    const int C = a->c1 + a->c2;
    pld_conv_args g = *a;
    g.x1 = dy;
    g.x2 = nullptr;
    g.c1 = a->cout;
    g.c2 = 0;
    g.h = g.oh = a->oh;
    g.w = g.ow = a->ow;
    g.sh = g.sw = 1;
    g.cout = C;
    g.in_scale = g.in_shift = nullptr;
    GemmConvParams p;
    int rc = fill_geom(&g, p);
    if (rc) return rc;
    float* t = (float*)a->ws;
    p.bmat = w_dgrad;
    p.bsplit = (const float*)a->w_split;
    p.M = (long)a->n * a->oh * a->ow;
    p.N = C;
    p.K = a->cout;
    p.bias = nullptr;
    p.out1 = t;
    p.ld1 = C;
    p.acc1 = 0;
    p.out2 = nullptr;
    p.ld2 = 0;
    p.acc2 = 0;
    p.split = C;
    const bool vec = (p.c1 % 4 == 0) && aligned16(dy) && aligned16(w_dgrad);
    const bool vec16 = vec && (p.c1 % 16 == 0);
    hipStream_t st = as_stream(stream);
    rc = run_fwd_gemm(p, vec, vec16, a->tile, (char*)a->ws + tb, a->ws_bytes - tb, st,
                      "pld_conv2d_dgrad", a->math);
    if (rc) return rc;
    const long total = (long)a->n * a->h * a->w * C;
    if (C % 4 == 0 && a->c1 % 4 == 0 && aligned16(t) && aligned16(dx1) &&
        (!dx2 || aligned16(dx2))) {
      if (accumulate1 && (!dx2 || accumulate2)) {
        const long tq = (long)a->n * a->oh * a->ow * (C / 4);
        stride_scatter4_acc_kernel<<<std::min<unsigned>(cdiv(tq, 256), 16384), 256, 0, st>>>(
            t, (int)tq, FastDiv((uint32_t)(C / 4)), FastDiv((uint32_t)a->ow),
            FastDiv((uint32_t)a->oh), a->h, a->w, a->sh, a->sw, C, dx1, a->c1, dx2);
        return check_launch("stride_scatter4_acc_kernel");
      }
      const int total4 = (int)(total / 4);
      stride_scatter4_kernel<<<std::min<unsigned>(cdiv(total4, 256), 16384), 256, 0, st>>>(
          t, total4, FastDiv((uint32_t)(C / 4)), FastDiv((uint32_t)a->w),
          FastDiv((uint32_t)a->h), a->oh, a->ow, a->sh, a->sw, C, dx1, a->c1, accumulate1, dx2,
          accumulate2);
      return check_launch("stride_scatter4_kernel");
    }
    stride_scatter_kernel<<<std::min<unsigned>(cdiv(total, 256), 16384), 256, 0, st>>>(
        t, a->n, a->h, a->w, a->oh, a->ow, a->sh, a->sw, C, dx1, a->c1, accumulate1, dx2,
        accumulate2);
    return check_launch("stride_scatter_kernel");
  }
  if (pld__scalar1x1_eligible(a) && aligned16(dy) && aligned16(dx1))
    return pld__scalar1x1_apply(dy, w_dgrad, nullptr, dx1, (long)a->n * a->h * a->w,
                                accumulate1, stream);
  if (pld__skinny_eligible(a) && aligned16(dx1))
    return pld__skinny_dgrad(a, dy, w_dgrad, dx1, accumulate1, stream);
  // 1x1: w_dgrad is [cin][cout], dx = dy . w_dgrad^T
  if (pld__thin_geom(a) && pld__thin_ok(a->cout, a->c1) && aligned16(dy) && aligned16(dx1) &&
      aligned16(w_dgrad))
    return pld__thin_gemm(dy, w_dgrad, nullptr, dx1, (long)a->n * a->h * a->w, a->cout, a->c1,
                          accumulate1, stream, nullptr);
  if (wide_conv(a, a->cout, a->c1) && aligned16(dy) && aligned16(w_dgrad) && aligned16(dx1))
    return pld__wide_gemm(dy, w_dgrad, nullptr, dx1, (long)a->n * a->h * a->w, a->cout, a->c1,
                          accumulate1, stream, nullptr);
  // dx[img][iy][ix][ci] = sum_{ty,tx,co} dy[img][iy+ty-pt'][ix+tx-pl'][co] * Wd[ci][ty][tx][co]
  // with pt' = kh-1-pt and the output spatial = the forward input spatial.
  pld_conv_args g = *a;
  g.x1 = dy;
  g.x2 = nullptr;
  g.c1 = a->cout;
  g.c2 = 0;
  g.h = a->oh;
  g.w = a->ow;
  g.oh = a->h;
  g.ow = a->w;
  g.pad_t = a->kh - 1 - a->pad_t;
  g.pad_l = a->kw - 1 - a->pad_l;
  g.cout = a->c1 + a->c2;
  g.in_scale = g.in_shift = nullptr;
  GemmConvParams p;
  int rc = fill_geom(&g, p);
  if (rc) return rc;
  p.bmat = w_dgrad;
  p.bsplit = (const float*)a->w_split;
  p.M = a->n * a->h * a->w;
  p.N = a->c1 + a->c2;
  p.K = a->kh * a->kw * a->cout;
  p.bias = nullptr;
  p.out1 = dx1;
  p.ld1 = a->c1;
  p.acc1 = accumulate1;
  p.out2 = dx2;
  p.ld2 = a->c2;
  p.acc2 = accumulate2;
  p.split = a->c1;
  const bool vec = (p.c1 % 4 == 0) && aligned16(dy) && aligned16(w_dgrad);
  const bool vec16 = vec && (p.c1 % 16 == 0);
  return run_fwd_gemm(p, vec, vec16, a->tile, a->ws, a->ws_bytes, as_stream(stream),
                      "pld_conv2d_dgrad", a->math);
}

// the bf16x3 patch WGRAD kernel's geometry (pld__x3_patch_wgrad_ok, from the call's args)
static bool wgrad_patch_geom(const pld_conv_args* a) {
  return a->kh == 3 && a->kw == 3 && a->sh == 1 && a->sw == 1 && a->in_scale == nullptr &&
         a->c1 % 16 == 0 && a->c2 % 16 == 0 && a->cout % 4 == 0 && a->pad_t >= 0 &&
         a->pad_t <= 2 && a->pad_l >= 0 && a->pad_l <= 2;
}

// stream_grid (optional): > 0 when the call runs the tile stream with that many workgroups
// (stream_p then holds its sk_* plan)
static void wgrad_plan(const pld_conv_args* a, int& M, int& N, long& K, int& splits,
                       int& kt_per, int& cfg, bool& x3, bool* patch_out = nullptr,
                       int* stream_grid = nullptr, GemmConvParams* stream_p = nullptr) {
  M = a->kh * a->kw * (a->c1 + a->c2);
  N = a->cout;
  K = (long)a->n * a->oh * a->ow;
  int tile;
  bool patch, stream;
  resolve_sched(a->math, x3_wgrad_geom(a->c1, a->c2, a->cout, a->in_scale != nullptr), a->tile,
                x3, tile, &patch, &stream);
  if (patch && !wgrad_patch_geom(a)) {
    patch = false;
    tile = -1;
  }
  if (patch_out) *patch_out = patch;
  if (stream_grid) *stream_grid = 0;
  if (stream) {  // whole-tensor descriptors: operands under 2 GiB
    const long in_bytes = (long)a->n * a->h * a->w * std::max(a->c1, a->c2) * 4;
    if (in_bytes < MAX_RECORDS && K * N * 4 < MAX_RECORDS) {
      GemmConvParams q{};
      q.M = M;
      q.N = N;
      cfg = tile;
      splits = 1;
      kt_per = 0;
      const int G = x3_stream_plan(q, cfg, (K + X3_BK - 1) / X3_BK);
      if (stream_grid) *stream_grid = G;
      if (stream_p) *stream_p = q;
      return;
    }
    tile = -1;
  }
  if (patch) {  // patch schedule: workgroups = chunks x cout tiles x splits, ~512 in all
    const long tiles = (long)cdiv(a->ow, 32) * cdiv(a->oh, pld__x3_patch_wgrad_th(N)) * a->n;
    const long blocks = (long)(cdiv(a->c1, 32) + cdiv(a->c2, 32)) *
                        cdiv(N, pld__x3_patch_wgrad_cw(N));
    long s = std::max<long>(1, (512 + blocks - 1) / blocks);
    s = std::min<long>(s, tiles);
    kt_per = (int)((tiles + s - 1) / s);
    splits = (int)((tiles + kt_per - 1) / kt_per);
    cfg = 0;
    return;
  }
  const int bk = x3 ? X3_BK : BK;
  const long ktiles = (K + bk - 1) / bk;
  // pick the tile for an unsplit GEMM, then split K until ~2-3 blocks per CU
  int bm = 0, bn = 0;
  if (x3) {
    int tm, tn, occ;
    cfg = x3_choose(M, N, K, tile, true);
    pld__x3_cfg_dims(cfg, &bm, &bn, &tm, &tn, &occ);
  } else {
    cfg = choose_tile(M, N, K, 1, tile);
    bm = kTiles[cfg].bm;
    bn = kTiles[cfg].bn;
  }
  const long tiles = (long)cdiv(M, bm) * cdiv(N, bn);
  long s = std::max<long>(1, ((x3 ? 512 : 768) + tiles - 1) / tiles);
  s = std::min<long>(s, std::max<long>(1, ktiles / (x3 ? 4 : 8)));  // >= 128 pixels per block
  // a workgroup's pixel range must stay within 32-bit buffer offsets of its base image
  const long img_in = (long)a->h * a->w * std::max(a->c1, a->c2) * 4;
  const long img_out = (long)a->oh * a->ow;
  for (;;) {
    const long kp = (ktiles + s - 1) / s;
    const long span_a = (kp * bk / img_out + 2) * img_in;
    const long span_b = kp * bk * (long)N * 4;
    if ((span_a < MAX_RECORDS && span_b < MAX_RECORDS) || kp <= 1) break;
    ++s;
  }
  kt_per = (int)((ktiles + s - 1) / s);
  splits = (int)((ktiles + kt_per - 1) / kt_per);
}

// split-K slabs + the first-level group partials of the two-level reduction
static size_t wgrad_ws_bytes(int splits, int M, int N) {
  if (splits <= 1) return 0;
  const int groups = splits > 2 * SPLIT_GROUP ? (splits + SPLIT_GROUP - 1) / SPLIT_GROUP : 0;
  return sizeof(float) * (size_t)(splits + groups) * M * N;
}

extern "C" size_t pld_conv2d_wgrad_workspace_size(const pld_conv_args* a) {
  if (!a || a->n <= 0 || a->kh <= 0 || a->kw <= 0 || a->c1 <= 0 || a->c2 < 0 || a->cout <= 0 ||
      a->oh <= 0 || a->ow <= 0)
    return 0;
  if (pld__scalar1x1_eligible(a)) return pld__scalar1x1_wgrad_ws();
  if (pld__skinny_eligible(a)) return pld__skinny_wgrad_ws(a);
  int M, N, splits, kt, cfg, G;
  long K;
  bool x3;
  GemmConvParams q{};
  wgrad_plan(a, M, N, K, splits, kt, cfg, x3, nullptr, &G, &q);
  if (G > 0) return x3_stream_slab_bytes(q, cfg, G);
  return wgrad_ws_bytes(splits, M, N);
}

extern "C" int pld_conv2d_wgrad(const pld_conv_args* a, const float* dy, float* dw,
                                int accumulate, void* ws, size_t ws_bytes, void* stream) {
  GemmConvParams p;
  int rc = fill_geom(a, p);
  if (rc) return rc;
  PLD_CHECK_ARG(dy && dw, "pld_conv2d_wgrad: null dy/dw");
  if (pld__scalar1x1_eligible(a) && aligned16(a->x1) && aligned16(dy)) {
    const size_t need = pld__scalar1x1_wgrad_ws();
    PLD_CHECK_ARG(ws && ws_bytes >= need, "pld_conv2d_wgrad: workspace %zu < %zu bytes",
                  ws_bytes, need);
    return pld__scalar1x1_wgrad(a->x1, dy, dw, (long)a->n * a->h * a->w, accumulate, ws, stream);
  }
  if (pld__skinny_eligible(a) && aligned16(a->x1)) {
    const size_t need = pld__skinny_wgrad_ws(a);
    PLD_CHECK_ARG(ws && ws_bytes >= need, "pld_conv2d_wgrad: workspace %zu < %zu bytes",
                  ws_bytes, need);
    return pld__skinny_wgrad(a, dy, dw, accumulate, ws, stream);
  }
  int M, N, splits, kt_per, cfg, sk_grid;
  long K;
  bool x3, patch;
  GemmConvParams sk{};
  wgrad_plan(a, M, N, K, splits, kt_per, cfg, x3, &patch, &sk_grid, &sk);
  PLD_CHECK_ARG(K < (1L << 31), "pld_conv2d_wgrad: too many pixels");
  const size_t need = sk_grid > 0 ? x3_stream_slab_bytes(sk, cfg, sk_grid)
                                  : wgrad_ws_bytes(splits, M, N);
  PLD_CHECK_ARG(ws_bytes >= need && (need == 0 || ws),
                "pld_conv2d_wgrad: workspace %zu < %zu bytes", ws_bytes, need);
  p.bmat = dy;
  p.M = M;
  p.N = N;
  p.K = (int)K;
  p.bias = nullptr;
  p.split = N;
  p.ktiles_per_split = kt_per;
  hipStream_t st = as_stream(stream);
  if (splits > 1) {
    p.out1 = (float*)ws;
    p.ld1 = N;
    p.acc1 = 0;
    p.zstride = (long)M * N;
  } else {
    p.out1 = dw;
    p.ld1 = N;
    p.acc1 = accumulate;
    p.zstride = 0;
  }
  const bool vec = (p.c1 % 4 == 0) && (p.c2 % 4 == 0) && aligned16(p.x1) &&
                   (!p.x2 || aligned16(p.x2)) && aligned16(dy) &&
                   (!p.in_scale || (aligned16(p.in_scale) && aligned16(p.in_shift)));
  if (patch) {
    PLD_CHECK_ARG(vec, "pld_conv2d_wgrad: bf16x3 operands must be 16-byte aligned");
    PLD_CHECK_ARG((long)a->h * a->w * std::max(a->c1, a->c2) * 4 < MAX_RECORDS &&
                      (long)a->oh * a->ow * N * 4 < MAX_RECORDS,
                  "pld_conv2d_wgrad: image too large for 32-bit buffer offsets");
    rc = pld__x3_patch_wgrad_launch(&p, splits, st);
  } else if (x3 && sk_grid > 0) {
    PLD_CHECK_ARG(vec, "pld_conv2d_wgrad: bf16x3 operands must be 16-byte aligned");
    p.sk_nk = sk.sk_nk;
    p.sk_tiles = sk.sk_tiles;
    p.sk_nnb = sk.sk_nnb;
    p.sk_align = sk.sk_align;
    p.sk_slab = sk.sk_align ? nullptr : (float*)ws;
    p.ktiles_per_split = 0;
    rc = pld__x3_launch(&p, MODE_WGRAD, 1, cfg, sk_grid, st);
  } else if (x3) {
    PLD_CHECK_ARG(vec, "pld_conv2d_wgrad: bf16x3 operands must be 16-byte aligned");
    rc = pld__x3_launch(&p, MODE_WGRAD, splits, cfg, 0, st);
  } else {
    rc = launch_igemm<MODE_WGRAD>(p, vec, false, splits, cfg, st);
  }
  if (rc || splits == 1) return rc;
  const long n = (long)M * N;
  const float* src = (const float*)ws;
  int terms = splits;
  if (splits > 2 * SPLIT_GROUP && splits <= 32 * SPLIT_GROUP) {
    const int groups = (splits + SPLIT_GROUP - 1) / SPLIT_GROUP;
    const int G = groups <= 4 ? 4 : groups <= 8 ? 8 : groups <= 16 ? 16 : 32;
    const unsigned blocks = (unsigned)cdiv(n, 256 / G);
    if (G == 4) splitk_reduce2_kernel<4><<<blocks, 256, 0, st>>>(src, splits, n, dw, accumulate);
    else if (G == 8) splitk_reduce2_kernel<8><<<blocks, 256, 0, st>>>(src, splits, n, dw, accumulate);
    else if (G == 16) splitk_reduce2_kernel<16><<<blocks, 256, 0, st>>>(src, splits, n, dw, accumulate);
    else splitk_reduce2_kernel<32><<<blocks, 256, 0, st>>>(src, splits, n, dw, accumulate);
    return check_launch("splitk_reduce2_kernel");
  }
  if (splits > 2 * SPLIT_GROUP) {
    const int groups = (splits + SPLIT_GROUP - 1) / SPLIT_GROUP;
    float* part = (float*)ws + (long)splits * n;
    splitk_group_kernel<<<dim3(cdiv(n, 256), groups), 256, 0, st>>>(src, splits, n, part);
    rc = check_launch("splitk_group_kernel");
    if (rc) return rc;
    src = part;
    terms = groups;
  }
  splitk_reduce_kernel<<<std::min<unsigned>(cdiv(n, 256), 4096), 256, 0, st>>>(
      src, terms, n, dw, accumulate);
  return check_launch("splitk_reduce_kernel");
}
