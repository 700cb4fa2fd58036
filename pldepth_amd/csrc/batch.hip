// Training-batch assembly from a device-resident dataset:
// pldepth/data/providers/hourglass_provider.py:29-62 zips (image, mask, gt), flips the three
// jointly left-right with p = 0.5 (:35-49), shuffles and batches. With the dataset in HBM a
// batch is one gather: output image b is source image idx[b], its width axis reversed pixel-wise
// when flip[b] != 0 (the c channels of a pixel keep their order). Pure copies, bit-exact.
//
// HBM-bound: ~128 MB in and ~128 MB out for 32 images of 448 x 448 (x3 + depth + mask). One
// launch covers the three arrays; a work item is one 16-byte vector of the output (the image's
// vectors first, then the depth maps', then the masks'), so the lanes of a wave store
// consecutive vectors, with streaming stores: the batch is read next by other kernels. An
// unflipped vector is one 16-byte load. A flipped one-channel row of w % 4 == 0 pixels reads the
// mirrored vector, which is aligned as well, and reverses it in registers; a flipped pixel of
// c = 3 floats straddles vectors, so those four floats are loaded one by one (the lanes of a
// wave still cover one contiguous span of the source row). Rows that do not split into aligned
// vectors (w % 4 != 0, c other than 1 or 3, a misaligned base) take the scalar kernel, one
// pixel per work item.
#include <algorithm>
#include <climits>

#include "common.h"

namespace pld {

struct BatchGeom {
  int h, w;
  unsigned total;         // work items (< 2^32 - grid size: B * h * w <= INT_MAX)
  unsigned n_img, n_map;  // of which the image's; one map's
  FastDiv img_row;        // items per image row; their dividends stay below 2^31
  FastDiv map_row;        // items per depth-map / mask row
  FastDiv rows;           // h
};

// source row of output row `row` = (b, y): image idx[b], row y
__device__ __forceinline__ long source_row(const BatchGeom& g, const int* __restrict__ idx,
                                           const int* __restrict__ flip, unsigned row,
                                           bool& flipped) {
  const unsigned b = g.rows.div(row), y = g.rows.mod(row, b);
  flipped = flip != nullptr && flip[b] != 0;
  return (long)idx[b] * g.h + y;
}

// vector q of a one-channel output row: the mirrored vector of the source row, reversed
__device__ __forceinline__ void move_map4(const float* __restrict__ srow, float* __restrict__ drow,
                                          int w, unsigned q, bool flipped) {
  const int dx = 4 * (int)q;
  float4 v = *reinterpret_cast<const float4*>(srow + (flipped ? w - 4 - dx : dx));
  if (flipped) v = make_float4(v.w, v.z, v.y, v.x);
  st_nt4(drow + dx, v);
}

// w % 4 == 0 and every base 16-byte aligned (checked by the launcher)
template <int C>
__global__ __launch_bounds__(256) void batch_gather_flip_vec_kernel(
    const float* __restrict__ imgs, const float* __restrict__ gts, const float* __restrict__ masks,
    const int* __restrict__ idx, const int* __restrict__ flip, BatchGeom g, float* __restrict__ x,
    float* __restrict__ gt, float* __restrict__ mask) {
  for (unsigned u = blockIdx.x * 256u + threadIdx.x; u < g.total; u += gridDim.x * 256u) {
    bool f;
    if (u < g.n_img) {
      const unsigned row = g.img_row.div(u), q = g.img_row.mod(u, row);
      const float* s = imgs + source_row(g, idx, flip, row, f) * g.w * C;
      float* d = x + (long)row * g.w * C;
      if (C == 1) {
        move_map4(s, d, g.w, q, f);
      } else if (!f) {
        st_nt4(d + 4 * q, *reinterpret_cast<const float4*>(s + 4 * q));
      } else {
        float e[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {  // element 4q + j of the row = channel ch of pixel p
          const unsigned el = 4 * q + j, p = el / C, ch = el - p * C;
          e[j] = s[(g.w - 1 - p) * C + ch];
        }
        st_nt4(d + 4 * q, make_float4(e[0], e[1], e[2], e[3]));
      }
    } else {
      unsigned t = u - g.n_img;
      const float* src = gts;
      float* dst = gt;
      if (gts == nullptr || t >= g.n_map) {  // the masks' items follow the depth maps', if any
        if (gts != nullptr) t -= g.n_map;
        src = masks, dst = mask;
      }
      const unsigned row = g.map_row.div(t), q = g.map_row.mod(t, row);
      const long srow = source_row(g, idx, flip, row, f);
      move_map4(src + srow * g.w, dst + (long)row * g.w, g.w, q, f);
    }
  }
}

// one pixel of the three arrays per work item, any w and c
__global__ __launch_bounds__(256) void batch_gather_flip_kernel(
    const float* __restrict__ imgs, const float* __restrict__ gts, const float* __restrict__ masks,
    const int* __restrict__ idx, const int* __restrict__ flip, BatchGeom g, int c,
    float* __restrict__ x, float* __restrict__ gt, float* __restrict__ mask) {
  for (unsigned u = blockIdx.x * 256u + threadIdx.x; u < g.total; u += gridDim.x * 256u) {
    bool f;
    const unsigned row = g.map_row.div(u), dx = g.map_row.mod(u, row);
    const long srow = source_row(g, idx, flip, row, f);
    const long s = srow * g.w + (f ? g.w - 1 - (int)dx : (int)dx);
    const long d = (long)row * g.w + dx;
    for (int ch = 0; ch < c; ++ch) x[d * c + ch] = imgs[s * c + ch];
    if (gts) gt[d] = gts[s];
    if (masks) mask[d] = masks[s];
  }
}

}  // namespace pld

using namespace pld;

extern "C" int pld_batch_gather_flip(const float* imgs, const float* gts, const float* masks,
                                     int n, int h, int w, int c, const int* idx, const int* flip,
                                     int B, float* x, float* gt, float* mask, void* stream) {
  PLD_CHECK_ARG(imgs && idx && x, "pld_batch_gather_flip: null pointer");
  PLD_CHECK_ARG(n > 0 && h > 0 && w > 0 && c > 0 && B > 0,
                "pld_batch_gather_flip: bad sizes n=%d h=%d w=%d c=%d B=%d", n, h, w, c, B);
  PLD_CHECK_ARG((gts != nullptr) == (gt != nullptr) && (masks != nullptr) == (mask != nullptr),
                "pld_batch_gather_flip: gts/gt and masks/mask are given together or not at all");
  const long pixels = (long)B * h * w;
  PLD_CHECK_ARG(pixels <= INT_MAX, "pld_batch_gather_flip: a batch of %ld pixels (limit 2^31 - 1)",
                pixels);
  const bool vec = w % 4 == 0 && (c == 1 || c == 3) && aligned16(imgs) && aligned16(x) &&
                   aligned16(gts) && aligned16(gt) && aligned16(masks) && aligned16(mask);
  const unsigned rows = (unsigned)B * h;
  BatchGeom g;
  g.h = h, g.w = w;
  g.rows = FastDiv((uint32_t)h);
  if (vec) {  // at most pixels * 5 / 4 items
    g.img_row = FastDiv((uint32_t)(w / 4 * c));
    g.map_row = FastDiv((uint32_t)(w / 4));
    g.n_img = rows * (w / 4 * c), g.n_map = rows * (w / 4);
    g.total = g.n_img + (gts ? g.n_map : 0) + (masks ? g.n_map : 0);
  } else {
    g.img_row = g.map_row = FastDiv((uint32_t)w);
    g.n_img = g.n_map = g.total = (unsigned)pixels;
  }
  // memory-bound: at most ~8 blocks per CU, the rest by grid stride
  const unsigned grid = std::min<unsigned>(cdiv(g.total, 256), 2048);
  hipStream_t st = as_stream(stream);
  if (vec && c == 3)
    batch_gather_flip_vec_kernel<3><<<grid, 256, 0, st>>>(imgs, gts, masks, idx, flip, g, x, gt,
                                                          mask);
  else if (vec)
    batch_gather_flip_vec_kernel<1><<<grid, 256, 0, st>>>(imgs, gts, masks, idx, flip, g, x, gt,
                                                          mask);
  else
    batch_gather_flip_kernel<<<grid, 256, 0, st>>>(imgs, gts, masks, idx, flip, g, c, x, gt, mask);
  return check_launch("batch_gather_flip_kernel");
}
