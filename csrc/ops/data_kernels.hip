// Device-resident image input pipeline (gfx950): one kernel turns rows of an HBM-resident uint8
// dataset [n][S][S][3] into the training batch the stem consumes -- gather (device permutation +
// device cursor), random crop, horizontal flip, normalisation, bf16 rounding and the stem's
// space-to-depth rearrangement in one pass over the batch's bytes. The fp32 image batch never
// exists. The CPU twin is arena_amd/ops/reference.py image_batch (bit for bit).
//
//   pos = cursor[0] * B + r                                  (batch row r)
//   training:   row = perm[pos % L]
//   evaluation: row = perm[pos] while pos < L, else padding (zero image, label -100, row -1)
//   training:   y0 = draw(0, S - Hc + 1), x0 = draw(1, S - Wc + 1), flip = hash(2) >> 31 with
//               hash(k) = hash4(seed, stream * 4 + k, low32(pos), high32(pos)) (common.h) and
//               draw(k, m) = (hash(k) * m) >> 32: functions of (seed, stream, pos) alone, so a
//               resumed run and a replayed graph draw the same values
//   evaluation: the centre crop, y0 = (S - Hc) / 2, x0 = (S - Wc) / 2, no flip
//   out pixel (y, x, c) = table[c][img[row][y0 + y][x0 + (flip ? Wc - 1 - x : x)][c]]
// table is 3 x 256 values of the output dtype, built once on the host from mean and std, so the
// kernel and the reference cannot round differently.
// image_batch_resized_kernel (below) is the training batch with a random resized crop in place of
// the fixed window and, in two launches, a colour distortion of the resampled bytes (CPU twin:
// image_batch_color).
#include "common.h"

namespace {

struct ImageRow {
  long long row;   // dataset row, -1: padding
  int y0, x0, flip;
};

// The same for every thread of a block (blockIdx.y is the batch row): scalar work.
__device__ __forceinline__ ImageRow image_row(const ArenaImageBatch& a, int r) {
  ImageRow o;
  const unsigned long long pos = (unsigned long long)a.cursor[0] * (unsigned long long)a.B + r;
  const unsigned long long L = (unsigned long long)a.L;
  if (a.train) {
    o.row = a.perm[pos % L];
    const uint32_t lo = (uint32_t)pos, hi = (uint32_t)(pos >> 32);
    const uint32_t st = (uint32_t)a.stream * 4u;
    o.y0 = (int)__umulhi(arena::hash4(a.seed, st + 0u, lo, hi), (uint32_t)(a.S - a.Hc + 1));
    o.x0 = (int)__umulhi(arena::hash4(a.seed, st + 1u, lo, hi), (uint32_t)(a.S - a.Wc + 1));
    o.flip = (int)(arena::hash4(a.seed, st + 2u, lo, hi) >> 31);
  } else {
    o.row = pos < L ? (long long)a.perm[pos] : -1;
    o.y0 = (a.S - a.Hc) >> 1;
    o.x0 = (a.S - a.Wc) >> 1;
    o.flip = 0;
  }
  // a permutation entry outside the dataset reads nothing: the row becomes padding
  if (o.row < 0 || o.row >= a.n) o.row = -1;
  return o;
}

// One thread per 2x2 pixel quad (i, j) of one batch row: two source runs of 6 bytes (rows
// 2i, 2i+1; pixels 2j, 2j+1), read bytewise because x0 is arbitrary.
//   LAYOUT 0 (s2d): z[b][i][j][(dy*2+dx)*3 + c], channels 12..15 zero: two 16-byte stores, the
//                   channel order of s2d_stem_kernel (conv_kernels.hip)
//   LAYOUT 1 (nhwc): x[b][2i+dy][2j+dx][c]: per dy the quad's 6 values are contiguous, stored
//                   as three 4-byte (bf16) or 8-byte (fp32) words, aligned because Wc is even
template <typename T, int LAYOUT>
__global__ __launch_bounds__(256) void image_batch_kernel(const ArenaImageBatch a) {
  __shared__ T tab[3 * 256];
  for (int e = threadIdx.x; e < 3 * 256; e += 256) tab[e] = ((const T*)a.table)[e];
  const int b = blockIdx.y;
  const ImageRow ir = image_row(a, b);
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    a.labels_out[b] = ir.row >= 0 ? a.labels[ir.row] : -100ll;
    a.rows_out[b] = (int)ir.row;
    a.crop_out[3 * b + 0] = ir.y0;
    a.crop_out[3 * b + 1] = ir.x0;
    a.crop_out[3 * b + 2] = ir.flip;
  }
  __syncthreads();
  const int Hz = a.Hc >> 1, Wz = a.Wc >> 1;
  const int q = blockIdx.x * 256 + threadIdx.x;
  if (q >= Hz * Wz) return;
  const int i = q / Wz, j = q - i * Wz;
  T v[12];   // [dy][dx][c]
  if (ir.row >= 0) {
    // the row's byte offset is 64-bit (n * S * S * 3 passes 2^31 at 10923 images of 256^2);
    // offsets inside one image fit 32 bits (S <= 16384, checked by the launcher)
    const uint8_t* img = a.images + (size_t)ir.row * ((size_t)a.S * a.S * 3);
    const int xa = ir.flip ? ir.x0 + a.Wc - 1 - 2 * j : ir.x0 + 2 * j;   // source of dx = 0
    const int xb = ir.flip ? xa - 1 : xa + 1;                            // source of dx = 1
#pragma unroll
    for (int dy = 0; dy < 2; ++dy) {
      const uint32_t rowoff = (uint32_t)(ir.y0 + 2 * i + dy) * (uint32_t)a.S;
      const uint8_t* pa = img + (rowoff + (uint32_t)xa) * 3u;
      const uint8_t* pb = img + (rowoff + (uint32_t)xb) * 3u;
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        v[dy * 6 + c] = tab[c * 256 + pa[c]];
        v[dy * 6 + 3 + c] = tab[c * 256 + pb[c]];
      }
    }
  } else {
#pragma unroll
    for (int k = 0; k < 12; ++k) v[k] = (T)0;
  }
  if constexpr (LAYOUT == 0) {
    static_assert(sizeof(T) == 2, "the space-to-depth tensor is bf16");
    uint4 o0, o1;
    o0.x = v[0] | ((uint32_t)v[1] << 16); o0.y = v[2] | ((uint32_t)v[3] << 16);
    o0.z = v[4] | ((uint32_t)v[5] << 16); o0.w = v[6] | ((uint32_t)v[7] << 16);
    o1.x = v[8] | ((uint32_t)v[9] << 16); o1.y = v[10] | ((uint32_t)v[11] << 16);
    o1.z = 0u; o1.w = 0u;
    uint4* dst = reinterpret_cast<uint4*>((uint16_t*)a.out + ((size_t)b * Hz * Wz + q) * 16);
    dst[0] = o0;
    dst[1] = o1;
  } else {
#pragma unroll
    for (int dy = 0; dy < 2; ++dy) {
      const size_t e = (((size_t)b * a.Hc + 2 * i + dy) * a.Wc + 2 * j) * 3;
      if constexpr (sizeof(T) == 2) {
        uint32_t* dst = reinterpret_cast<uint32_t*>((uint16_t*)a.out + e);
#pragma unroll
        for (int k = 0; k < 3; ++k)
          dst[k] = (uint32_t)v[dy * 6 + 2 * k] | ((uint32_t)v[dy * 6 + 2 * k + 1] << 16);
      } else {
        float2* dst = reinterpret_cast<float2*>((float*)a.out + e);
#pragma unroll
        for (int k = 0; k < 3; ++k) dst[k] = make_float2(v[dy * 6 + 2 * k], v[dy * 6 + 2 * k + 1]);
      }
    }
  }
}

// ---- random resized crop: a box of random area and aspect ratio, resized to Hc x Wc ----
//   box = draw(3, T), (h, w) = boxes[box] clamped to [2, S], y0 = draw(0, S - h + 1),
//   x0 = draw(1, S - w + 1), flip = hash(2) >> 31
//   output row y reads box rows i0, i1 with weights 256 - f, f (image_tap: bilinear, half-pixel
//   centres, 8-bit weights); columns alike, of xs = flip ? Wc - 1 - x : x
//   u = ((256-fx)(256-fy) p00 + fx (256-fy) p01 + (256-fx) fy p10 + fx fy p11 + 32768) >> 16
//   out pixel (y, x, c) = table[c][u]
// Integers only (all below 2^32 for S <= 16384), so the CPU twin (reference.py
// image_batch_resized) matches bit for bit; with (h, w) == (Hc, Wc) every f is 0 and i0 = y: the
// fixed crop above.
struct ImageBox {
  long long row;   // dataset row, -1: padding
  int y0, x0, flip, h, w;
};

// The same for every thread of a block, as image_row.
__device__ __forceinline__ ImageBox image_box(const ArenaImageBatch& a, const int* boxes,
                                              int n_boxes, int r) {
  ImageBox o;
  const unsigned long long pos = (unsigned long long)a.cursor[0] * (unsigned long long)a.B + r;
  o.row = a.perm[pos % (unsigned long long)a.L];
  const uint32_t lo = (uint32_t)pos, hi = (uint32_t)(pos >> 32);
  const uint32_t st = (uint32_t)a.stream * 4u;
  const uint32_t t = __umulhi(arena::hash4(a.seed, st + 3u, lo, hi), (uint32_t)n_boxes);
  // the loader checks the table; a stray entry is clamped, so no tap can leave the image
  o.h = min(max(boxes[2 * t], 2), a.S);
  o.w = min(max(boxes[2 * t + 1], 2), a.S);
  o.y0 = (int)__umulhi(arena::hash4(a.seed, st + 0u, lo, hi), (uint32_t)(a.S - o.h + 1));
  o.x0 = (int)__umulhi(arena::hash4(a.seed, st + 1u, lo, hi), (uint32_t)(a.S - o.w + 1));
  o.flip = (int)(arena::hash4(a.seed, st + 2u, lo, hi) >> 31);
  if (o.row < 0 || o.row >= a.n) o.row = -1;
  return o;
}

struct ImageTap {
  uint32_t i0, i1, f;   // source indices in [0, extent) and the weight of i1 (of 256)
};

// Output index o of n reads a source of `extent` samples: i0 <= extent - 1 because
// (2 o + 1) extent - n < 2 n extent.
__device__ __forceinline__ ImageTap image_tap(int o, int n, int extent) {
  ImageTap t;
  const int num = (2 * o + 1) * extent - n;
  if (num < 0) {
    t.i0 = 0u;
    t.f = 0u;
  } else {
    const uint32_t den = 2u * (uint32_t)n;
    t.i0 = (uint32_t)num / den;
    t.f = (((uint32_t)num - t.i0 * den) * 256u) / den;
  }
  t.i1 = min(t.i0 + 1u, (uint32_t)extent - 1u);
  return t;
}

// ---- colour distortion (tf_cnn_benchmarks' distort_color, YIQ form) on the resampled bytes ----
//   m = cdraw(0, T), k = k_lo + cdraw(1, k_hi - k_lo + 1), d = cdraw(2, 2 D + 1) - D with
//   cdraw(i, n) = draw(i, n) under the seed a.seed ^ kColorSeedSalt (draws 0..3 stay as they are)
//   per image: s_c = sum of u_c over the Hc x Wc crop, A = k M[m] (Q20),
//              b_c = d 2^20 + floor((256 - k) (M[m] s)_c / (Hc Wc))            (64-bit)
//   per pixel: v_c = clamp((A u + b + 2^19)_c >> 20, 0, 255), then table[c][v_c]
// The contract, its rounding rule and the 32-bit width argument: ops/reference.py
// (image_batch_color, the CPU twin, bit for bit). s_c needs the whole crop before any pixel is
// written, so a first launch of the same grid stores each block's channel sums (plain stores of
// integers: nothing to re-zero between replays, no order to depend on) and every block of the
// second launch adds up its image's row of them.
constexpr uint32_t kColorSeedSalt = 0x636F6C72u;

struct ImageColorDraw {
  int m, k, d;
};

// The same for every thread of a block, as image_box.
__device__ __forceinline__ ImageColorDraw image_color_draw(const ArenaImageBatch& a,
                                                           const ArenaImageColor& col, int r) {
  ImageColorDraw o;
  const unsigned long long pos = (unsigned long long)a.cursor[0] * (unsigned long long)a.B + r;
  const uint32_t lo = (uint32_t)pos, hi = (uint32_t)(pos >> 32);
  const uint32_t seed = a.seed ^ kColorSeedSalt, st = (uint32_t)a.stream * 4u;
  o.m = (int)__umulhi(arena::hash4(seed, st + 0u, lo, hi), (uint32_t)col.n_matrices);
  o.k = col.k_lo + (int)__umulhi(arena::hash4(seed, st + 1u, lo, hi),
                                 (uint32_t)(col.k_hi - col.k_lo + 1));
  o.d = (int)__umulhi(arena::hash4(seed, st + 2u, lo, hi), (uint32_t)(2 * col.delta + 1)) -
        col.delta;
  return o;
}

// coef[0..8] = A (row-major), coef[9..11] = b for batch row b, computed once per block: every
// thread adds a share of the image's block sums, threads 0..2 finish one channel each. Ends with
// a barrier.
__device__ __forceinline__ void image_color_coefficients(const ArenaImageBatch& a,
                                                         const ArenaImageColor& col,
                                                         const ImageColorDraw& cd, int b,
                                                         int* coef) {
  __shared__ long long red[4][3];
  long long s[3] = {0ll, 0ll, 0ll};
  const int* row = col.sums + (size_t)b * gridDim.x * 3;
  for (int e = threadIdx.x; e < (int)gridDim.x; e += 256) {
#pragma unroll
    for (int c = 0; c < 3; ++c) s[c] += row[3 * e + c];
  }
#pragma unroll
  for (int c = 0; c < 3; ++c) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) s[c] += __shfl_down(s[c], off);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6][c] = s[c];
  }
  __syncthreads();
  if (threadIdx.x < 3) {
    const int c = threadIdx.x;
    const int* M = col.matrices + 9 * cd.m + 3 * c;
    long long t = 0;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      t += (long long)M[k] * (red[0][k] + red[1][k] + red[2][k] + red[3][k]);
      coef[3 * c + k] = cd.k * M[k];
    }
    const long long num = (long long)(256 - cd.k) * t, N = (long long)a.Hc * a.Wc;
    long long quo = num / N;
    if (num - quo * N < 0) --quo;   // floor, as the reference's //
    coef[9 + c] = cd.d * (1 << 20) + (int)quo;
  }
  __syncthreads();
}

// The sums launch: col.sums[b][blockIdx.x][c] = the sum of channel c over this block's quads (at
// most 1024 pixels of at most 255: 32 bits hold it); zero for a padding row.
__device__ __forceinline__ void image_store_block_sums(uint32_t s[3], int* sums, int b) {
  __shared__ uint32_t red[4][3];
#pragma unroll
  for (int c = 0; c < 3; ++c) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) s[c] += __shfl_down(s[c], off);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6][c] = s[c];
  }
  __syncthreads();
  if (threadIdx.x < 3) {
    const int c = threadIdx.x;
    sums[((size_t)b * gridDim.x + blockIdx.x) * 3 + c] =
        (int)(red[0][c] + red[1][c] + red[2][c] + red[3][c]);
  }
}

// Grid, LDS table, quad per thread, output forms and padding rows as image_batch_kernel. Each of
// the quad's 4 pixels reads its own 4 taps of 3 bytes (a box larger than the crop shares none),
// all 48 loads issued before the first table lookup.
// MODE picks what happens to the resampled byte u: IMAGE_PLAIN looks it up in the table;
// IMAGE_SUMS (T and LAYOUT unused) only adds it to the block's channel sums and writes no batch;
// IMAGE_COLOR distorts it with the coefficients made from those sums, then looks it up. One body,
// so the three cannot resample differently; every difference is an `if constexpr`, and the plain
// instantiations compile to the instructions they had before the colour distortion existed.
enum { IMAGE_PLAIN = 0, IMAGE_SUMS = 1, IMAGE_COLOR = 2 };

template <typename T, int LAYOUT, int MODE>
__global__ __launch_bounds__(256) void image_batch_resized_kernel(const ArenaImageBatch a,
                                                                  const int* boxes, int n_boxes,
                                                                  int* box_out,
                                                                  const ArenaImageColor col) {
  __shared__ T tab[3 * 256];
  __shared__ int coef[MODE == IMAGE_COLOR ? 12 : 1];
  if constexpr (MODE != IMAGE_SUMS)
    for (int e = threadIdx.x; e < 3 * 256; e += 256) tab[e] = ((const T*)a.table)[e];
  const int b = blockIdx.y;
  const ImageBox ib = image_box(a, boxes, n_boxes, b);
  ImageColorDraw cd{};
  if constexpr (MODE == IMAGE_COLOR) cd = image_color_draw(a, col, b);
  if (MODE != IMAGE_SUMS && blockIdx.x == 0 && threadIdx.x == 0) {
    a.labels_out[b] = ib.row >= 0 ? a.labels[ib.row] : -100ll;
    a.rows_out[b] = (int)ib.row;
    a.crop_out[3 * b + 0] = ib.y0;
    a.crop_out[3 * b + 1] = ib.x0;
    a.crop_out[3 * b + 2] = ib.flip;
    box_out[2 * b + 0] = ib.h;
    box_out[2 * b + 1] = ib.w;
    if constexpr (MODE == IMAGE_COLOR) {
      col.color_out[3 * b + 0] = cd.m;
      col.color_out[3 * b + 1] = cd.k;
      col.color_out[3 * b + 2] = cd.d;
    }
  }
  if constexpr (MODE == IMAGE_COLOR) image_color_coefficients(a, col, cd, b, coef);
  if constexpr (MODE == IMAGE_PLAIN) __syncthreads();
  const int Hz = a.Hc >> 1, Wz = a.Wc >> 1;
  const int q = blockIdx.x * 256 + threadIdx.x;
  // the sums launch keeps every thread for its reduction
  if (MODE != IMAGE_SUMS && q >= Hz * Wz) return;
  const int i = q / Wz, j = q - i * Wz;
  T v[12];   // [dy][dx][c]
  uint32_t ub[12];                 // IMAGE_COLOR: the bytes before the table
  uint32_t s[3] = {0u, 0u, 0u};    // IMAGE_SUMS: this thread's channel sums
  if (ib.row >= 0 && (MODE != IMAGE_SUMS || q < Hz * Wz)) {
    const uint8_t* img = a.images + (size_t)ib.row * ((size_t)a.S * a.S * 3);
    ImageTap ty[2], tx[2];
#pragma unroll
    for (int d = 0; d < 2; ++d) {
      ty[d] = image_tap(2 * i + d, a.Hc, ib.h);
      tx[d] = image_tap(ib.flip ? a.Wc - 1 - 2 * j - d : 2 * j + d, a.Wc, ib.w);
    }
    uint32_t p[2][2][4][3];   // [dy][dx][tap 00, 01, 10, 11][c]
#pragma unroll
    for (int dy = 0; dy < 2; ++dy) {
      const uint32_t r0 = ((uint32_t)ib.y0 + ty[dy].i0) * (uint32_t)a.S + (uint32_t)ib.x0;
      const uint32_t r1 = ((uint32_t)ib.y0 + ty[dy].i1) * (uint32_t)a.S + (uint32_t)ib.x0;
#pragma unroll
      for (int dx = 0; dx < 2; ++dx) {
        const uint8_t* t00 = img + (r0 + tx[dx].i0) * 3u;
        const uint8_t* t01 = img + (r0 + tx[dx].i1) * 3u;
        const uint8_t* t10 = img + (r1 + tx[dx].i0) * 3u;
        const uint8_t* t11 = img + (r1 + tx[dx].i1) * 3u;
#pragma unroll
        for (int c = 0; c < 3; ++c) {
          p[dy][dx][0][c] = t00[c];
          p[dy][dx][1][c] = t01[c];
          p[dy][dx][2][c] = t10[c];
          p[dy][dx][3][c] = t11[c];
        }
      }
    }
#pragma unroll
    for (int dy = 0; dy < 2; ++dy) {
#pragma unroll
      for (int dx = 0; dx < 2; ++dx) {
        const uint32_t fy = ty[dy].f, fx = tx[dx].f;
        const uint32_t w00 = (256u - fx) * (256u - fy), w01 = fx * (256u - fy);
        const uint32_t w10 = (256u - fx) * fy, w11 = fx * fy;   // the four sum to 65536
#pragma unroll
        for (int c = 0; c < 3; ++c) {
          const uint32_t u = (w00 * p[dy][dx][0][c] + w01 * p[dy][dx][1][c] +
                              w10 * p[dy][dx][2][c] + w11 * p[dy][dx][3][c] + 32768u) >> 16;
          if constexpr (MODE == IMAGE_SUMS)
            s[c] += u;
          else if constexpr (MODE == IMAGE_COLOR)
            ub[dy * 6 + dx * 3 + c] = u;
          else
            v[dy * 6 + dx * 3 + c] = tab[c * 256 + u];
        }
      }
    }
    if constexpr (MODE == IMAGE_COLOR) {
      int A[12];
#pragma unroll
      for (int k = 0; k < 12; ++k) A[k] = coef[k];
#pragma unroll
      for (int px = 0; px < 4; ++px) {
        const int u0 = (int)ub[3 * px], u1 = (int)ub[3 * px + 1], u2 = (int)ub[3 * px + 2];
#pragma unroll
        for (int c = 0; c < 3; ++c) {
          // >> of a negative sum rounds towards minus infinity, as the reference's
          const int acc = A[3 * c] * u0 + A[3 * c + 1] * u1 + A[3 * c + 2] * u2 + A[9 + c] +
                          (1 << 19);
          v[3 * px + c] = tab[c * 256 + min(max(acc >> 20, 0), 255)];
        }
      }
    }
  } else {
#pragma unroll
    for (int k = 0; k < 12; ++k) v[k] = (T)0;
  }
  if constexpr (MODE == IMAGE_SUMS) {
    image_store_block_sums(s, col.sums, b);
  } else if constexpr (LAYOUT == 0) {
    static_assert(sizeof(T) == 2, "the space-to-depth tensor is bf16");
    uint4 o0, o1;
    o0.x = v[0] | ((uint32_t)v[1] << 16); o0.y = v[2] | ((uint32_t)v[3] << 16);
    o0.z = v[4] | ((uint32_t)v[5] << 16); o0.w = v[6] | ((uint32_t)v[7] << 16);
    o1.x = v[8] | ((uint32_t)v[9] << 16); o1.y = v[10] | ((uint32_t)v[11] << 16);
    o1.z = 0u; o1.w = 0u;
    uint4* dst = reinterpret_cast<uint4*>((uint16_t*)a.out + ((size_t)b * Hz * Wz + q) * 16);
    dst[0] = o0;
    dst[1] = o1;
  } else {
#pragma unroll
    for (int dy = 0; dy < 2; ++dy) {
      const size_t e = (((size_t)b * a.Hc + 2 * i + dy) * a.Wc + 2 * j) * 3;
      if constexpr (sizeof(T) == 2) {
        uint32_t* dst = reinterpret_cast<uint32_t*>((uint16_t*)a.out + e);
#pragma unroll
        for (int k = 0; k < 3; ++k)
          dst[k] = (uint32_t)v[dy * 6 + 2 * k] | ((uint32_t)v[dy * 6 + 2 * k + 1] << 16);
      } else {
        float2* dst = reinterpret_cast<float2*>((float*)a.out + e);
#pragma unroll
        for (int k = 0; k < 3; ++k) dst[k] = make_float2(v[dy * 6 + 2 * k], v[dy * 6 + 2 * k + 1]);
      }
    }
  }
}

// A launch of its own, in stream order after the batch kernel: no block of that launch can see
// the advanced cursor.
__global__ void image_cursor_kernel(long long* cursor) { cursor[0] += 1; }

bool image_batch_args_ok(const ArenaImageBatch& a, int layout, int out_f32) {
  return !(a.B < 1 || a.B > 65535 || a.n < 1 || a.L < 1 || a.S < 2 || a.S > 16384 || a.Hc < 2 ||
           a.Wc < 2 || (a.Hc & 1) || (a.Wc & 1) || a.Hc > a.S || a.Wc > a.S || a.stream < 0 ||
           a.stream >= (1 << 30) || layout < 0 || layout > 1 || (layout == 0 && out_f32));
}

}  // namespace

// layout 0: space-to-depth z (bf16), 1: nhwc; out_f32: the nhwc output (and the table) is fp32,
// else bf16. advance: add 1 to the device cursor after the batch is written.
extern "C" hipError_t arena_image_batch(ArenaImageBatch a, int layout, int out_f32, int advance,
                                        hipStream_t st) {
  if (!image_batch_args_ok(a, layout, out_f32)) return hipErrorInvalidValue;
  const int quads = (a.Hc / 2) * (a.Wc / 2);
  const dim3 g((unsigned)((quads + 255) / 256), (unsigned)a.B);
  if (layout == 0)
    hipLaunchKernelGGL((image_batch_kernel<uint16_t, 0>), g, dim3(256), 0, st, a);
  else if (out_f32)
    hipLaunchKernelGGL((image_batch_kernel<float, 1>), g, dim3(256), 0, st, a);
  else
    hipLaunchKernelGGL((image_batch_kernel<uint16_t, 1>), g, dim3(256), 0, st, a);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess || !advance) return e;
  hipLaunchKernelGGL(image_cursor_kernel, dim3(1), dim3(1), 0, st, a.cursor);
  return hipGetLastError();
}

// The training batch with a random resized crop (a.train must be 1): boxes [n_boxes][2] are the
// candidate (h, w) in source pixels, box_out [B][2] receives the drawn one. Otherwise as above.
extern "C" hipError_t arena_image_batch_resized(ArenaImageBatch a, const int* boxes, int n_boxes,
                                                int* box_out, int layout, int out_f32,
                                                int advance, hipStream_t st) {
  if (!image_batch_args_ok(a, layout, out_f32) || !a.train || n_boxes < 1 || n_boxes > 4096)
    return hipErrorInvalidValue;
  const int quads = (a.Hc / 2) * (a.Wc / 2);
  const dim3 g((unsigned)((quads + 255) / 256), (unsigned)a.B);
  if (layout == 0)
    hipLaunchKernelGGL((image_batch_resized_kernel<uint16_t, 0, IMAGE_PLAIN>), g, dim3(256), 0, st,
                       a, boxes, n_boxes, box_out, ArenaImageColor{});
  else if (out_f32)
    hipLaunchKernelGGL((image_batch_resized_kernel<float, 1, IMAGE_PLAIN>), g, dim3(256), 0, st, a,
                       boxes, n_boxes, box_out, ArenaImageColor{});
  else
    hipLaunchKernelGGL((image_batch_resized_kernel<uint16_t, 1, IMAGE_PLAIN>), g, dim3(256), 0, st,
                       a, boxes, n_boxes, box_out, ArenaImageColor{});
  hipError_t e = hipGetLastError();
  if (e != hipSuccess || !advance) return e;
  hipLaunchKernelGGL(image_cursor_kernel, dim3(1), dim3(1), 0, st, a.cursor);
  return hipGetLastError();
}

// The resized training batch with the colour distortion: arena_image_batch_resized's operands plus
// `col` (abi.h). Two launches of the same grid, the channel sums and then the batch, before the
// cursor's.
extern "C" hipError_t arena_image_batch_color(ArenaImageBatch a, const int* boxes, int n_boxes,
                                              int* box_out, ArenaImageColor col, int layout,
                                              int out_f32, int advance, hipStream_t st) {
  if (!image_batch_args_ok(a, layout, out_f32) || !a.train || n_boxes < 1 || n_boxes > 4096 ||
      col.n_matrices < 1 || col.n_matrices > 4096 || col.k_lo < 0 || col.k_hi < col.k_lo ||
      col.k_hi > 4096 || col.delta < 0 || col.delta > 255)
    return hipErrorInvalidValue;
  const int quads = (a.Hc / 2) * (a.Wc / 2);
  const dim3 g((unsigned)((quads + 255) / 256), (unsigned)a.B);
  hipLaunchKernelGGL((image_batch_resized_kernel<uint16_t, 0, IMAGE_SUMS>), g, dim3(256), 0, st, a,
                     boxes, n_boxes, box_out, col);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  if (layout == 0)
    hipLaunchKernelGGL((image_batch_resized_kernel<uint16_t, 0, IMAGE_COLOR>), g, dim3(256), 0, st,
                       a, boxes, n_boxes, box_out, col);
  else if (out_f32)
    hipLaunchKernelGGL((image_batch_resized_kernel<float, 1, IMAGE_COLOR>), g, dim3(256), 0, st, a,
                       boxes, n_boxes, box_out, col);
  else
    hipLaunchKernelGGL((image_batch_resized_kernel<uint16_t, 1, IMAGE_COLOR>), g, dim3(256), 0, st,
                       a, boxes, n_boxes, box_out, col);
  e = hipGetLastError();
  if (e != hipSuccess || !advance) return e;
  hipLaunchKernelGGL(image_cursor_kernel, dim3(1), dim3(1), 0, st, a.cursor);
  return hipGetLastError();
}
