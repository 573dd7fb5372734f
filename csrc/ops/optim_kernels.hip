// Optimizer kernels for gfx950 (MI355X): everything that turns gradients into weights outside the
// fused MNIST step, plus the one-lane clocks that feed them.
//
//   adam_flat / sgd_flat   Adam / plain SGD over one flat fp32 parameter buffer (after the
//                          gradient all-reduce)
//   mt_copy_scale          multi-tensor flatten/unflatten with scale (gradient buckets)
//   mt_master<RULE>        multi-tensor update, master layout: bf16 gradients, fp32 masters and
//                          states, rounded bf16 weights written for the next forward
//   mt_f32<RULE>           multi-tensor update, fp32 layout: fp32 gradients and weights, any sizes
//   mt_lars_norms/_update  LARS over the master layout: per-tensor norms, then mt_master's SGD
//   shard_sgd<BF16>        momentum SGD over one flat range, either layout
//   shard_update<RULE, L>  RMSProp / Adam / Nesterov SGD over one flat range in the master, fp32
//                          or wide layout (fp32 gradient, fp32 master, bf16 weights written);
//                          plain SGD in the wide one
//   shard_lars_*           LARS over the pieces of a rank's shard: norms, [all-reduce], update
//   lr_schedule, adam_tick the learning-rate schedule and Adam's bias correction, on the device
//
// The multi-tensor kernels share ONE walk (mt_chunk: which tensor owns this 1024-element chunk),
// ONE 4 x bf16 pack / unpack, ONE body per layout (master_update4 / f32_update4) and ONE host
// loop (mt_fill + mt_launch_groups); a RULE (SgdRule, SgdScaledRule, NesterovRule,
// NesterovScaledRule, RmspropRule, AdamRule) is the per-element arithmetic and the number of fp32
// state buffers it keeps.
#include "common.h"
#include "adam.h"

#include <algorithm>
#include <vector>

using namespace arena;

namespace {

// ---------------------------------------------------------------------------------------------
// adam_flat: float4-vectorised Adam over the flat parameter buffer; n must be a multiple of 4.
// ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void adam_flat_kernel(float* __restrict__ P, float* __restrict__ Mm,
                                                        float* __restrict__ V,
                                                        const float* __restrict__ G, long long n4,
                                                        ArenaAdam a, ArenaCounterOp ctr) {
  counter_op(ctr);
  const AdamCoef co = adam_coef(a);
  for (long long i = blockIdx.x * 256LL + threadIdx.x; i < n4; i += (long long)gridDim.x * 256) {
    float4 p = reinterpret_cast<float4*>(P)[i];
    float4 m = reinterpret_cast<float4*>(Mm)[i];
    float4 v = reinterpret_cast<float4*>(V)[i];
    const float4 g = reinterpret_cast<const float4*>(G)[i];
    adam_apply(co, g.x, p.x, m.x, v.x);
    adam_apply(co, g.y, p.y, m.y, v.y);
    adam_apply(co, g.z, p.z, m.z, v.z);
    adam_apply(co, g.w, p.w, m.w, v.w);
    reinterpret_cast<float4*>(P)[i] = p;
    reinterpret_cast<float4*>(Mm)[i] = m;
    reinterpret_cast<float4*>(V)[i] = v;
  }
}

__global__ __launch_bounds__(256) void sgd_flat_kernel(float* __restrict__ P,
                                                       const float* __restrict__ G, long long n4,
                                                       float lr, const float* lr_ptr, float gscale) {
  const float l = lr_ptr ? *lr_ptr : lr;
  for (long long i = blockIdx.x * 256LL + threadIdx.x; i < n4; i += (long long)gridDim.x * 256) {
    float4 p = reinterpret_cast<float4*>(P)[i];
    const float4 g = reinterpret_cast<const float4*>(G)[i];
    p.x -= l * g.x * gscale; p.y -= l * g.y * gscale; p.z -= l * g.z * gscale; p.w -= l * g.w * gscale;
    reinterpret_cast<float4*>(P)[i] = p;
  }
}

// ---------------------------------------------------------------------------------------------
// The multi-tensor walk. A launch covers up to kMtMax tensors; tensor i owns the 1024-element
// chunks [blk_begin[i], blk_begin[i + 1]) of the launch, one block each (mt_lars_norms_kernel: one
// wave each). ptr[i] is the tensor outside the flat buffer (a gradient; mt_copy_scale: either
// side), off[i] / n[i] its segment of the flat buffers.
// ---------------------------------------------------------------------------------------------
constexpr int kMtMax = 48;
struct MtArgs {
  float* ptr[kMtMax];
  long long off[kMtMax];
  long long n[kMtMax];
  int blk_begin[kMtMax + 1];
  int count;
};

// Tensor that owns `chunk`; j0: the chunk's first element in it.
__device__ __forceinline__ int mt_chunk(const MtArgs& a, int chunk, long long& j0) {
  int ti = 0;
  for (int i = 1; i < a.count; ++i)
    if (chunk >= a.blk_begin[i]) ti = i;
  j0 = (long long)(chunk - a.blk_begin[ti]) * 1024;
  return ti;
}

// ---------------------------------------------------------------------------------------------
// mt_copy_scale: multi-tensor gather/scatter between a list of tensors and one flat bucket.
//   dir 0: flat[off_i + j] = src_i[j] * scale      (flatten gradients into the all-reduce bucket)
//   dir 1: dst_i[j] = flat[off_i + j] * scale      (unflatten reduced gradients)
// ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void mt_copy_scale_kernel(MtArgs a, float* __restrict__ flat,
                                                            float scale, int dir) {
  long long base;
  const int ti = mt_chunk(a, (int)blockIdx.x, base);
  float* t = a.ptr[ti];
  float* f = flat + a.off[ti];
  for (int k = 0; k < 4; ++k) {
    const long long j = base + k * 256 + threadIdx.x;
    if (j < a.n[ti]) {
      if (dir == 0) f[j] = t[j] * scale;
      else t[j] = f[j] * scale;
    }
  }
}

// ---------------------------------------------------------------------------------------------
// bf16 <-> fp32, four at a time (8 bytes of bf16 against 16 of fp32).
// ---------------------------------------------------------------------------------------------
__device__ inline float bf16_to_f32(uint32_t v) { return __uint_as_float(v << 16); }
__device__ inline uint32_t f32_to_bf16(float f) {
  uint32_t u = __float_as_uint(f);
  if ((u & 0x7fffffffu) > 0x7f800000u) return (u >> 16) | 0x40u;  // quiet NaN
  u += 0x7fffu + ((u >> 16) & 1u);                                  // round to nearest even
  return u >> 16;
}
__device__ __forceinline__ void bf16x4_unpack(uint2 g2, float g[4]) {
  g[0] = bf16_to_f32(g2.x & 0xffffu);
  g[1] = bf16_to_f32(g2.x >> 16);
  g[2] = bf16_to_f32(g2.y & 0xffffu);
  g[3] = bf16_to_f32(g2.y >> 16);
}
__device__ __forceinline__ uint2 bf16x4_pack(const uint32_t r[4]) {  // r: f32_to_bf16 results
  return make_uint2(r[0] | (r[1] << 16), r[2] | (r[3] << 16));
}

// ---------------------------------------------------------------------------------------------
// The update rules. Each is the arithmetic of ONE element (g: gradient, w: weight, s0 / s1: its
// fp32 states, step: the launch's step size) and kStates, the state buffers it keeps: a rule with
// one never touches s1, and the bodies below then issue no load or store for it.
//
//   SgdRule        torch.optim.SGD (dampening 0, no nesterov) as the master layout runs it:
//                  m = mu * m + (g + wd * w); w -= step * m. No scale factor: see below.
//   SgdScaledRule  the same with a gradient scale, in the order of the xGMI kernels' shard update
//                  (csrc/ccl/xgmi_ccl.hip xgmi_sgd_*): d = g * scale + wd * w; m = mu * m + d;
//                  w -= step * m. The fp32 layout and shard_sgd, both dtypes.
//   NesterovRule / NesterovScaledRule  the two above with Nesterov momentum (TF's
//                  use_nesterov=True, torch's nesterov=True with dampening 0;
//                  arena_amd/ops/reference.py defines it): the same d and m, then
//                  w = w - step * (d + mu * m). One state, which means what the plain rules' does.
//   RmspropRule / AdamRule  TF1's forms (arena_amd/ops/reference.py defines them). Both start from
//                  the coupled gradient d = g * scale + wd * w (scale is 1 on the master path):
//     RMSProp (s0 = ms, s1 = mom):  ms = rho * ms + omr * (d * d)
//                                   mom = mu * mom + lr * d / sqrt(ms + eps);  w = w - mom
//     Adam    (s0 = m,  s1 = v):    m = b1 * m + omb1 * d;  v = b2 * v + omb2 * (d * d)
//                                   w = w - (lr * corr) * m / (sqrt(v) + eps)
// omr / omb1 / omb2 are 1 - rho / 1 - b1 / 1 - b2 formed by the host in fp64: the fp32 difference
// 1 - float(0.999) is 4.7e-5 off. corr is the bias correction arena_adam_tick keeps on the device.
//
// SgdRule is not SgdScaledRule with scale = 1: this unit is built with -ffp-contract=fast, under
// which the compiler chooses, per expression shape, which products it fuses into an FMA and which
// it rounds on their own (g * scale + wd * w may become fma(g, scale, wd * w); g + wd * w has only
// one product to fuse). Each rule keeps its own text; tools/optim_bits.py compares two builds' bits.
// NesterovRule / NesterovScaledRule are two texts for the same reason.
// ---------------------------------------------------------------------------------------------
struct SgdRule {
  static constexpr int kStates = 1;
  static constexpr bool kCorr = false;
  static __device__ __forceinline__ void apply(float g, float& w, float& m, float&, float step,
                                               const ArenaOptHyper& h) {
    m = h.b * m + (g + h.wd * w);
    w = w - step * m;
  }
};

struct SgdScaledRule {
  static constexpr int kStates = 1;
  static constexpr bool kCorr = false;
  static __device__ __forceinline__ void apply(float g, float& w, float& m, float&, float step,
                                               const ArenaOptHyper& h) {
    const float d = g * h.scale + h.wd * w;
    m = h.b * m + d;
    w = w - step * m;
  }
};

struct NesterovRule {
  static constexpr int kStates = 1;
  static constexpr bool kCorr = false;
  static __device__ __forceinline__ void apply(float g, float& w, float& m, float&, float step,
                                               const ArenaOptHyper& h) {
    const float d = g + h.wd * w;
    m = h.b * m + d;
    w = w - step * (d + h.b * m);
  }
};

struct NesterovScaledRule {
  static constexpr int kStates = 1;
  static constexpr bool kCorr = false;
  static __device__ __forceinline__ void apply(float g, float& w, float& m, float&, float step,
                                               const ArenaOptHyper& h) {
    const float d = g * h.scale + h.wd * w;
    m = h.b * m + d;
    w = w - step * (d + h.b * m);
  }
};

struct RmspropRule {
  static constexpr int kStates = 2;
  static constexpr bool kCorr = false;
  static __device__ __forceinline__ void apply(float g, float& w, float& s0, float& s1, float step,
                                               const ArenaOptHyper& h) {
    const float d = g * h.scale + h.wd * w;
    s0 = h.a * s0 + h.oma * (d * d);
    s1 = h.b * s1 + step * d / sqrtf(s0 + h.eps);
    w = w - s1;
  }
};

struct AdamRule {
  static constexpr int kStates = 2;
  static constexpr bool kCorr = true;
  static __device__ __forceinline__ void apply(float g, float& w, float& s0, float& s1, float step,
                                               const ArenaOptHyper& h) {
    const float d = g * h.scale + h.wd * w;
    s0 = h.a * s0 + h.oma * d;
    s1 = h.b * s1 + h.omb * (d * d);
    w = w - step * s0 / (sqrtf(s1) + h.eps);
  }
};

// The per-launch step size: the learning rate (the device one when set: schedules under graph
// replay), times corr for Adam.
template <class RULE>
__device__ __forceinline__ float opt_step_size(const ArenaOptHyper& h) {
  const float lr = h.lr_ptr ? *h.lr_ptr : h.lr;
  if constexpr (RULE::kCorr) return lr * *h.corr;
  return lr;
}

// Master layout (mixed-precision CNN training), one thread's 4 elements: g points at 4 bf16
// gradients (autograd-owned, same storage order as the parameter), w / s0 / s1 / wbf at the same
// 4 elements of the flat buffers. One pass reads the bf16 grad + fp32 master + fp32 states and
// writes master, states and the rounded bf16 weight the next forward consumes, so autocast needs
// no per-step weight/grad casts: 22 bytes per element with one state, 28 with two. The bf16
// rounding stays INSIDE the element loop: with it after the loop the compiler pairs the products
// into other packed multiplies / FMAs and the low bits of the states move (measured; see
// shard_sgd_kernel).
template <class RULE>
__device__ __forceinline__ void master_update4(const uint16_t* g, float* w, float* s0, float* s1,
                                               uint16_t* wbf, float step, const ArenaOptHyper& h) {
  const uint2 g2 = *reinterpret_cast<const uint2*>(g);
  float4 w4 = *reinterpret_cast<const float4*>(w);
  float4 p4 = *reinterpret_cast<const float4*>(s0);
  float4 q4 = make_float4(0.f, 0.f, 0.f, 0.f);
  if constexpr (RULE::kStates == 2) q4 = *reinterpret_cast<const float4*>(s1);
  float gf[4];
  bf16x4_unpack(g2, gf);
  float* wf = &w4.x;
  float* p = &p4.x;
  float* q = &q4.x;
  uint32_t r[4];
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    RULE::apply(gf[k], wf[k], p[k], q[k], step, h);
    r[k] = f32_to_bf16(wf[k]);
  }
  *reinterpret_cast<float4*>(w) = w4;
  *reinterpret_cast<float4*>(s0) = p4;
  if constexpr (RULE::kStates == 2) *reinterpret_cast<float4*>(s1) = q4;
  *reinterpret_cast<uint2*>(wbf) = bf16x4_pack(r);
}

// fp32 layout, one thread's 4 elements through 16-byte accesses (all pointers 16-byte aligned).
template <class RULE>
__device__ __forceinline__ void f32_update4(const float* g, float* w, float* s0, float* s1,
                                            float step, const ArenaOptHyper& h) {
  const float4 g4 = *reinterpret_cast<const float4*>(g);
  float4 w4 = *reinterpret_cast<const float4*>(w);
  float4 p4 = *reinterpret_cast<const float4*>(s0);
  float4 q4 = make_float4(0.f, 0.f, 0.f, 0.f);
  if constexpr (RULE::kStates == 2) q4 = *reinterpret_cast<const float4*>(s1);
  RULE::apply(g4.x, w4.x, p4.x, q4.x, step, h);
  RULE::apply(g4.y, w4.y, p4.y, q4.y, step, h);
  RULE::apply(g4.z, w4.z, p4.z, q4.z, step, h);
  RULE::apply(g4.w, w4.w, p4.w, q4.w, step, h);
  *reinterpret_cast<float4*>(w) = w4;
  *reinterpret_cast<float4*>(s0) = p4;
  if constexpr (RULE::kStates == 2) *reinterpret_cast<float4*>(s1) = q4;
}

// Multi-tensor update over the master layout. Tensor i: bf16 gradient at a.ptr[i], master / state
// / bf16-param segments at a.off[i] of the flat buffers; n % 4 == 0 and offsets % 4 == 0.
template <class RULE>
__global__ __launch_bounds__(256) void mt_master_kernel(MtArgs a, float* __restrict__ master,
                                                        float* __restrict__ st0,
                                                        float* __restrict__ st1,
                                                        uint16_t* __restrict__ wbf,
                                                        ArenaOptHyper h) {
  const float step = opt_step_size<RULE>(h);
  long long j;
  const int ti = mt_chunk(a, (int)blockIdx.x, j);
  j += threadIdx.x * 4;
  if (j >= a.n[ti]) return;  // n % 4 == 0 (host-checked): a live thread owns 4 whole elements
  const long long o = a.off[ti] + j;
  master_update4<RULE>(reinterpret_cast<const uint16_t*>(a.ptr[ti]) + j, master + o, st0 + o,
                       st1 + o, wbf + o, step, h);
}

// Multi-tensor update over fp32 tensors with fp32 gradients (BatchNorm scales/shifts, biases):
// gradient at a.ptr[i], weight/state segment at a.off[i] of the flat buffers. Any n and any
// offset: a thread's 4 elements go through 16-byte accesses when all four exist and the segment
// and the gradient are 16-byte aligned, else one by one.
template <class RULE>
__global__ __launch_bounds__(256) void mt_f32_kernel(MtArgs a, float* __restrict__ wflat,
                                                     float* __restrict__ st0,
                                                     float* __restrict__ st1, ArenaOptHyper h) {
  const float step = opt_step_size<RULE>(h);
  long long j;
  const int ti = mt_chunk(a, (int)blockIdx.x, j);
  j += threadIdx.x * 4;
  const long long n = a.n[ti];
  if (j >= n) return;
  const float* g = a.ptr[ti] + j;
  float* w = wflat + a.off[ti] + j;
  float* p = st0 + a.off[ti] + j;
  float* q = st1 + a.off[ti] + j;
  // the flat buffers are 16-byte aligned (host-checked), so the segment is when its offset is
  const bool vec = j + 4 <= n && (a.off[ti] & 3) == 0 &&
                   (reinterpret_cast<uintptr_t>(a.ptr[ti]) & 15) == 0;
  if (vec) {
    f32_update4<RULE>(g, w, p, q, step, h);
  } else {
    for (int k = 0; k < 4 && j + k < n; ++k) {
      float wk = w[k], pk = p[k], qk = 0.f;
      if constexpr (RULE::kStates == 2) qk = q[k];
      RULE::apply(g[k], wk, pk, qk, step, h);
      w[k] = wk;
      p[k] = pk;
      if constexpr (RULE::kStates == 2) q[k] = qk;
    }
  }
}

// Momentum SGD over ONE flat range: a data-parallel rank's shard of a gradient bucket after the
// RCCL reduce-scatter (ShardedMasterSGD's off-node backend), SgdScaledRule in either layout.
// BF16: bf16 summed gradient, fp32 master, rounded bf16 weight written to wbf; else fp32 gradient
// and the fp32 weights are their own masters. n % 4 == 0 and 16-byte aligned fp32 pointers
// (host-checked): one thread owns 4 elements per grid-stride step.
// The bf16 body is master_update4's, written out: it rounds to bf16 AFTER its element loop, where
// master_update4 rounds inside it, and under -ffp-contract=fast that shape decides how the
// compiler pairs the products into packed multiplies and FMAs (here fma(wd, w, g * scale) two
// elements at a time; there mu * m and wd * w in one packed multiply, then plain adds). Each kernel
// keeps the shape, and so the bits, it has always had. For the same reason the numbers arrive as
// scalars, as arena_shard_sgd takes them: as one ArenaOptHyper argument, wd lies next to scale and
// the compiler multiplied (wd * w1, scale * g0) as a pair, rounding odd elements another way.
template <bool BF16>
__global__ __launch_bounds__(256) void shard_sgd_kernel(const void* __restrict__ grad,
                                                        float* __restrict__ w32,
                                                        float* __restrict__ mom,
                                                        uint16_t* __restrict__ wbf, long long n,
                                                        float lr, const float* lr_ptr, float mu,
                                                        float wd, float scale) {
  ArenaOptHyper h{};
  h.lr = lr;
  h.lr_ptr = lr_ptr;
  h.b = mu;
  h.wd = wd;
  h.scale = scale;
  const float step = opt_step_size<SgdScaledRule>(h);
  const long long stride = (long long)gridDim.x * 1024;
  for (long long j = ((long long)blockIdx.x * 256 + threadIdx.x) * 4; j < n; j += stride) {
    if constexpr (BF16) {
      float g[4], none = 0.f;
      const uint16_t* gp = reinterpret_cast<const uint16_t*>(grad) + j;
      bf16x4_unpack(*reinterpret_cast<const uint2*>(gp), g);
      float4 w4 = *reinterpret_cast<const float4*>(w32 + j);
      float4 m4 = *reinterpret_cast<const float4*>(mom + j);
      float* w = &w4.x;
      float* m = &m4.x;
#pragma unroll
      for (int k = 0; k < 4; ++k) SgdScaledRule::apply(g[k], w[k], m[k], none, step, h);
      *reinterpret_cast<float4*>(w32 + j) = w4;
      *reinterpret_cast<float4*>(mom + j) = m4;
      const uint32_t r[4] = {f32_to_bf16(w[0]), f32_to_bf16(w[1]), f32_to_bf16(w[2]),
                             f32_to_bf16(w[3])};
      *reinterpret_cast<uint2*>(wbf + j) = bf16x4_pack(r);
    } else {
      f32_update4<SgdScaledRule>(reinterpret_cast<const float*>(grad) + j, w32 + j, mom + j,
                                 nullptr, step, h);
    }
  }
}

// Wide layout, one thread's 4 elements: fp32 gradient (a reduce-scatter that summed in fp32), fp32
// master and states, rounded bf16 weights written. master_update4 with a 16-byte gradient load.
template <class RULE>
__device__ __forceinline__ void wide_update4(const float* g, float* w, float* s0, float* s1,
                                             uint16_t* wbf, float step, const ArenaOptHyper& h) {
  const float4 g4 = *reinterpret_cast<const float4*>(g);
  float4 w4 = *reinterpret_cast<const float4*>(w);
  float4 p4 = *reinterpret_cast<const float4*>(s0);
  float4 q4 = make_float4(0.f, 0.f, 0.f, 0.f);
  if constexpr (RULE::kStates == 2) q4 = *reinterpret_cast<const float4*>(s1);
  const float* gf = &g4.x;
  float* wf = &w4.x;
  float* p = &p4.x;
  float* q = &q4.x;
  uint32_t r[4];
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    RULE::apply(gf[k], wf[k], p[k], q[k], step, h);
    r[k] = f32_to_bf16(wf[k]);
  }
  *reinterpret_cast<float4*>(w) = w4;
  *reinterpret_cast<float4*>(s0) = p4;
  if constexpr (RULE::kStates == 2) *reinterpret_cast<float4*>(s1) = q4;
  *reinterpret_cast<uint2*>(wbf) = bf16x4_pack(r);
}

// The three layouts of a shard update: what the reduce-scatter left, and where the weights go.
enum { SHARD_MASTER = 0,  // bf16 gradient, fp32 master and states, bf16 weights written
       SHARD_F32 = 1,     // fp32 gradient, the fp32 weights are their own masters
       SHARD_WIDE = 2 };  // fp32 gradient, fp32 master and states, bf16 weights written

template <class RULE, int LAYOUT>
__device__ __forceinline__ void shard_update4(const void* grad, long long gj, float* w, float* s0,
                                              float* s1, uint16_t* wbf, float step,
                                              const ArenaOptHyper& h) {
  if constexpr (LAYOUT == SHARD_MASTER)
    master_update4<RULE>(reinterpret_cast<const uint16_t*>(grad) + gj, w, s0, s1, wbf, step, h);
  else if constexpr (LAYOUT == SHARD_F32)
    f32_update4<RULE>(reinterpret_cast<const float*>(grad) + gj, w, s0, s1, step, h);
  else
    wide_update4<RULE>(reinterpret_cast<const float*>(grad) + gj, w, s0, s1, wbf, step, h);
}

// RULE over ONE flat range in one of the three layouts: shard_sgd_kernel's grid-stride walk (one
// thread owns 4 elements per step; n % 4 == 0 and aligned pointers, host-checked) for the rules
// and the layout it does not know. A rule with one state never touches st1.
template <class RULE, int LAYOUT>
__global__ __launch_bounds__(256) void shard_update_kernel(const void* __restrict__ grad,
                                                           float* __restrict__ w32,
                                                           float* __restrict__ st0,
                                                           float* __restrict__ st1,
                                                           uint16_t* __restrict__ wbf, long long n,
                                                           ArenaOptHyper h) {
  const float step = opt_step_size<RULE>(h);
  const long long stride = (long long)gridDim.x * 1024;
  for (long long j = ((long long)blockIdx.x * 256 + threadIdx.x) * 4; j < n; j += stride)
    shard_update4<RULE, LAYOUT>(grad, j, w32 + j, st0 + j, st1 + j, wbf + j, step, h);
}

// The learning-rate schedule of arena_amd/ops/schedule.py, advanced on the device so a captured
// step changes its lr from replay to replay. One lane: finds the segment of *step by a linear
// search over the (at most 64) segments, evaluates it in fp64 exactly as reference_lr does (every
// operation rounded on its own: no contraction), rounds once to fp32, then counts the step.
__global__ void lr_schedule_kernel(const long long* __restrict__ seg, int n_seg,
                                   long long* __restrict__ step, float* __restrict__ lr) {
  // This unit is built with -ffp-contract=fast, under which the backend fuses a multiply into a
  // following add whatever `#pragma clang fp contract(off)` or __dmul_rn / __dadd_rn (a plain
  // `*` / `+` in HIP's headers) say. The empty asm below makes the product an opaque value, so
  // it is rounded on its own.
  if (blockIdx.x != 0 || threadIdx.x != 0) return;
  const long long t = *step;
  int k = 0;
  for (int i = 1; i < n_seg; ++i)
    if (t >= seg[4 * i]) k = i;
  const long long b = seg[4 * k], e = seg[4 * k + 1];
  const double lr0 = __longlong_as_double(seg[4 * k + 2]);
  const double lr1 = __longlong_as_double(seg[4 * k + 3]);
  double v = lr1;                        // the open-ended last segment holds its lr1
  if (k < n_seg - 1) {
    v = lr0;
    if (lr1 != lr0) {
      const double frac = (double)(t - b) / (double)(e - b);
      double rise = (lr1 - lr0) * frac;
      asm volatile("" : "+v"(rise));
      v = lr0 + rise;
    }
  }
  *lr = (float)v;
  *step = t + 1;
}

// Adam's clock (arena_amd/ops/optim.py AdamClock), advanced on the device so a captured step
// keeps correcting the bias from replay to replay. One lane: pw[0] = b1^t and pw[1] = b2^t as
// running fp64 products, corr = float(sqrt(1 - b2^t) / (1 - b1^t)) with every fp64 operation
// rounded on its own, exactly as reference_adam_corr does in Python floats. As in
// lr_schedule_kernel, the empty asm keeps -ffp-contract=fast from fusing each product into the
// subtraction that follows it.
__global__ void adam_tick_kernel(long long* __restrict__ step, double* __restrict__ pw,
                                 float* __restrict__ corr, double b1, double b2) {
  if (blockIdx.x != 0 || threadIdx.x != 0) return;
  double p1 = pw[0] * b1;
  double p2 = pw[1] * b2;
  asm volatile("" : "+v"(p1));
  asm volatile("" : "+v"(p2));
  pw[0] = p1;
  pw[1] = p2;
  *corr = (float)(sqrt(1.0 - p2) / (1.0 - p1));
  *step = *step + 1;
}

// ---------------------------------------------------------------------------------------------
// LARS (arena_amd/ops/reference.py defines it): momentum SGD over bf16 gradients with fp32
// masters whose step is lr * trust, trust = eeta * |w| / (|g| + wd * |w| + eps) per tensor. Two
// launches per group of 48 tensors over mt_master_kernel's walk (1024 elements per block):
//   mt_lars_norms_kernel   one wave per chunk writes part[chunk] = (sum w^2, sum g^2): 16 serial
//                          fp32 terms per lane, then the wave64 xor tree.
//   mt_lars_update_kernel  every block sums ITS tensor's partials in fp64 (lane t takes partials
//                          t, t + 256, ... in order, then the same tree), forms trust and applies
//                          mt_master_kernel<SgdRule>'s update with step = lr * trust.
// No atomics and nothing to zero: every partial is overwritten at every step. All blocks of a
// tensor run the same sums over the same values in the same order, so they hold the same trust
// bit for bit; the tensor's first block stores it to trust[slot].
// ---------------------------------------------------------------------------------------------
struct LarsSlots {
  int slot[kMtMax];  // trust[slot[i]] receives tensor i's trust ratio
  int part_base;     // this launch group's first (w^2, g^2) pair in the workspace
};

__device__ __forceinline__ double wave_sum_f64(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

// trust = eeta * wn / ((gn + wd * wn) + eps), 1 when a norm is 0: fp32 operations in the
// reference's order; as in lr_schedule_kernel, the empty asm keeps -ffp-contract=fast from fusing
// a product into the sum that follows it.
__device__ __forceinline__ float lars_trust(float wn, float gn, const ArenaOptHyper& h) {
  float trust = 1.f;
  if (wn > 0.f && gn > 0.f) {
    float num = h.a * wn;
    float dec = h.wd * wn;
    asm volatile("" : "+v"(num));
    asm volatile("" : "+v"(dec));
    trust = num / ((gn + dec) + h.eps);
  }
  return trust;
}

// A block's fp64 sums of `nb` (w^2, g^2) partials: lane t takes partials t, t + 256, ... in index
// order (4 loads in flight), then the wave64 xor tree, then the four waves in order. Every block
// that runs it over the same partials holds the same bits. red: 8 doubles of LDS.
__device__ __forceinline__ void block_sum_pairs(const float2* __restrict__ p, int nb, double* red,
                                                double& sw_out, double& sg_out) {
  double sw = 0.0, sg = 0.0;
  for (int i = threadIdx.x; i < nb; i += 1024) {
    float2 v[4];
#pragma unroll
    for (int k = 0; k < 4; ++k)
      v[k] = i + k * 256 < nb ? p[i + k * 256] : make_float2(0.f, 0.f);
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      sw += (double)v[k].x;
      sg += (double)v[k].y;
    }
  }
  sw = wave_sum_f64(sw);
  sg = wave_sum_f64(sg);
  if ((threadIdx.x & 63) == 0) {
    red[threadIdx.x >> 6] = sw;
    red[4 + (threadIdx.x >> 6)] = sg;
  }
  __syncthreads();
  sw_out = ((red[0] + red[1]) + red[2]) + red[3];
  sg_out = ((red[4] + red[5]) + red[6]) + red[7];
}

__global__ __launch_bounds__(256) void mt_lars_norms_kernel(MtArgs a, LarsSlots s,
                                                            const float* __restrict__ master,
                                                            float2* __restrict__ part) {
  // one wave per 1024-element chunk (the update kernel's block): no LDS, no barrier
  const int chunk = __builtin_amdgcn_readfirstlane((int)(blockIdx.x * 4 + (threadIdx.x >> 6)));
  if (chunk >= a.blk_begin[a.count]) return;
  long long j0;
  const int ti = mt_chunk(a, chunk, j0);
  j0 += (threadIdx.x & 63) * 4;
  const long long n = a.n[ti];
  const uint16_t* gp = reinterpret_cast<const uint16_t*>(a.ptr[ti]);
  const float* wp = master + a.off[ti];
  uint2 g2[4];
  float4 w4[4];
#pragma unroll
  for (int k = 0; k < 4; ++k) {  // n % 4 == 0 (host-checked): 4 whole elements or none
    const long long j = j0 + k * 256;
    const bool live = j < n;
    g2[k] = live ? *reinterpret_cast<const uint2*>(gp + j) : make_uint2(0u, 0u);
    w4[k] = live ? *reinterpret_cast<const float4*>(wp + j) : make_float4(0.f, 0.f, 0.f, 0.f);
  }
  float sw = 0.f, sg = 0.f;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    float g[4];
    bf16x4_unpack(g2[k], g);
    const float* w = &w4[k].x;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      sw += w[e] * w[e];
      sg += g[e] * g[e];
    }
  }
  sw = wave_sum(sw);
  sg = wave_sum(sg);
  if ((threadIdx.x & 63) == 0) part[s.part_base + chunk] = make_float2(sw, sg);
}

// h: lr / lr_ptr, b = momentum, wd, a = eeta, eps (ArenaOptHyper's LARS column).
__global__ __launch_bounds__(256) void mt_lars_update_kernel(
    MtArgs a, LarsSlots s, float* __restrict__ master, float* __restrict__ mom,
    uint16_t* __restrict__ wbf, const float2* __restrict__ part, float* __restrict__ trust_out,
    ArenaOptHyper h) {
  __shared__ double red[8];
  const float lr = opt_step_size<SgdRule>(h);
  long long j;
  const int ti = mt_chunk(a, (int)blockIdx.x, j);
  j += threadIdx.x * 4;
  const int first = a.blk_begin[ti];
  const int nb = a.blk_begin[ti + 1] - first;
  double sw, sg;
  block_sum_pairs(part + s.part_base + first, nb, red, sw, sg);
  const float wn = (float)sqrt(sw);
  const float gn = (float)sqrt(sg);
  const float trust = lars_trust(wn, gn, h);
  float step = lr * trust;
  asm volatile("" : "+v"(step));
  if ((int)blockIdx.x == first && threadIdx.x == 0) trust_out[s.slot[ti]] = trust;
  if (j >= a.n[ti]) return;  // n % 4 == 0 (host-checked): a live thread owns 4 whole elements
  const long long o = a.off[ti] + j;
  master_update4<SgdRule>(reinterpret_cast<const uint16_t*>(a.ptr[ti]) + j, master + o, mom + o,
                          nullptr, wbf + o, step, h);
}

// ---------------------------------------------------------------------------------------------
// Sharded LARS (ShardedMasterSGD rule="lars"): a rank's shard of a reduce-scattered sub-range
// intersects several tensors; each intersection is a PIECE of the walk above (a.ptr[i]: its summed
// gradient inside the shard, bf16 or, WIDE, fp32; a.off[i] / a.n[i]: its fp32 masters; s.slot[i]:
// its tensor's index in the sub-range). The norms are those of the averaged gradient d = g * scale
// (an fp32 product), summed over ALL ranks' pieces of a tensor, so the step is three parts:
//   shard_lars_part_kernel  mt_lars_norms_kernel over pieces: part[chunk] = (sum w^2, sum d^2)
//   shard_lars_sums_kernel  one block per piece: its partials in fp64 (block_sum_pairs' fixed
//                           order) to sums[2 * slot], sums[2 * slot + 1]
//   -- the host all-reduces sums (fp64, SUM): every rank then holds the same bits --
//   shard_lars_trust_kernel trust[slot] for every tensor of the sub-range, from the reduced sums
//   shard_lars_update_kernel every block forms its piece's trust the same way and applies
//                           SgdScaledRule with step = lr * trust
// Slots without a piece on this rank hold 0.0: f64_zero_kernel writes all of sums first. No
// atomics; the same bits on every run.
// ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void f64_zero_kernel(double* __restrict__ v, int n) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i < n) v[i] = 0.0;
}

template <bool WIDE>
__global__ __launch_bounds__(256) void shard_lars_part_kernel(MtArgs a, int part_base,
                                                              const float* __restrict__ master,
                                                              float scale,
                                                              float2* __restrict__ part) {
  // one wave per 1024-element chunk, as mt_lars_norms_kernel: no LDS, no barrier
  const int chunk = __builtin_amdgcn_readfirstlane((int)(blockIdx.x * 4 + (threadIdx.x >> 6)));
  if (chunk >= a.blk_begin[a.count]) return;
  long long j0;
  const int ti = mt_chunk(a, chunk, j0);
  j0 += (threadIdx.x & 63) * 4;
  const long long n = a.n[ti];
  const float* wp = master + a.off[ti];
  float4 g4[4], w4[4];
#pragma unroll
  for (int k = 0; k < 4; ++k) {  // n % 4 == 0 (host-checked): 4 whole elements or none
    const long long j = j0 + k * 256;
    const bool live = j < n;
    g4[k] = make_float4(0.f, 0.f, 0.f, 0.f);
    if (live) {
      if constexpr (WIDE) {
        g4[k] = *reinterpret_cast<const float4*>(a.ptr[ti] + j);
      } else {
        const uint16_t* gp = reinterpret_cast<const uint16_t*>(a.ptr[ti]);
        bf16x4_unpack(*reinterpret_cast<const uint2*>(gp + j), &g4[k].x);
      }
    }
    w4[k] = live ? *reinterpret_cast<const float4*>(wp + j) : make_float4(0.f, 0.f, 0.f, 0.f);
  }
  float sw = 0.f, sg = 0.f;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const float* g = &g4[k].x;
    const float* w = &w4[k].x;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const float d = g[e] * scale;
      sw += w[e] * w[e];
      sg += d * d;
    }
  }
  sw = wave_sum(sw);
  sg = wave_sum(sg);
  if ((threadIdx.x & 63) == 0) part[part_base + chunk] = make_float2(sw, sg);
}

__global__ __launch_bounds__(256) void shard_lars_sums_kernel(MtArgs a, LarsSlots s,
                                                              const float2* __restrict__ part,
                                                              double* __restrict__ sums) {
  __shared__ double red[8];
  const int ti = blockIdx.x;  // one block per piece
  const int first = a.blk_begin[ti];
  double sw, sg;
  block_sum_pairs(part + s.part_base + first, a.blk_begin[ti + 1] - first, red, sw, sg);
  if (threadIdx.x == 0) {
    sums[2 * s.slot[ti]] = sw;
    sums[2 * s.slot[ti] + 1] = sg;
  }
}

__global__ __launch_bounds__(256) void shard_lars_trust_kernel(const double* __restrict__ sums,
                                                               float* __restrict__ trust,
                                                               int n_slots, ArenaOptHyper h) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i < n_slots)
    trust[i] = lars_trust((float)sqrt(sums[2 * i]), (float)sqrt(sums[2 * i + 1]), h);
}

// h: lr / lr_ptr, b = momentum, wd, a = eeta, eps, scale (ArenaOptHyper's LARS column + scale).
template <bool WIDE>
__global__ __launch_bounds__(256) void shard_lars_update_kernel(
    MtArgs a, LarsSlots s, float* __restrict__ master, float* __restrict__ mom,
    uint16_t* __restrict__ wbf, const double* __restrict__ sums, ArenaOptHyper h) {
  const float lr = opt_step_size<SgdScaledRule>(h);
  long long j;
  const int ti = mt_chunk(a, (int)blockIdx.x, j);
  j += threadIdx.x * 4;
  const int slot = s.slot[ti];
  const float trust = lars_trust((float)sqrt(sums[2 * slot]), (float)sqrt(sums[2 * slot + 1]), h);
  float step = lr * trust;
  asm volatile("" : "+v"(step));
  if (j >= a.n[ti]) return;  // n % 4 == 0 (host-checked): a live thread owns 4 whole elements
  const long long o = a.off[ti] + j;
  shard_update4<SgdScaledRule, WIDE ? SHARD_WIDE : SHARD_MASTER>(a.ptr[ti], j, master + o, mom + o,
                                                                 nullptr, wbf + o, step, h);
}

// ---------------------------------------------------------------------------------------------
// Host side: any number of tensors, kMtMax per launch.
// ---------------------------------------------------------------------------------------------
// Fills MtArgs for tensors [base, base + cnt) and returns the launch's block count.
inline int mt_fill(MtArgs& a, const void* const* ptrs, const long long* offs, const long long* ns,
                   int base, int cnt) {
  int blocks = 0;
  for (int i = 0; i < cnt; ++i) {
    a.ptr[i] = const_cast<float*>(reinterpret_cast<const float*>(ptrs[base + i]));
    a.off[i] = offs[base + i];
    a.n[i] = ns[base + i];
    a.blk_begin[i] = blocks;
    blocks += (int)((ns[base + i] + 1023) / 1024);
  }
  a.blk_begin[cnt] = blocks;
  a.count = cnt;
  return blocks;
}

// launch(a, blocks, base, cnt) -> hipError_t once per group of kMtMax tensors that has any block.
// The caller validates ALL tensors before calling this: no group runs ahead of a bad argument.
template <class LAUNCH>
hipError_t mt_launch_groups(const void* const* ptrs, const long long* offs, const long long* ns,
                            int count, LAUNCH&& launch) {
  for (int base = 0; base < count; base += kMtMax) {
    MtArgs a;
    const int cnt = std::min(kMtMax, count - base);
    const int blocks = mt_fill(a, ptrs, offs, ns, base, cnt);
    if (blocks == 0) continue;
    const hipError_t e = launch(a, blocks, base, cnt);
    if (e != hipSuccess) return e;
  }
  return hipSuccess;
}

// Segment sizes and offsets: never negative; the master layout's are multiples of 4.
inline bool mt_segments_ok(const long long* offs, const long long* ns, int count, int multiple) {
  for (int i = 0; i < count; ++i)
    if (ns[i] < 0 || offs[i] < 0 || ns[i] % multiple || offs[i] % multiple) return false;
  return true;
}

template <class RULE>
hipError_t launch_master(const void* const* grads, const long long* offs, const long long* ns,
                         int count, float* master, float* st0, float* st1, void* wbf,
                         const ArenaOptHyper& h, hipStream_t stream) {
  return mt_launch_groups(grads, offs, ns, count, [&](const MtArgs& a, int blocks, int, int) {
    hipLaunchKernelGGL(mt_master_kernel<RULE>, dim3(blocks), dim3(256), 0, stream, a, master, st0,
                       st1, reinterpret_cast<uint16_t*>(wbf), h);
    return hipGetLastError();
  });
}

template <class RULE>
hipError_t launch_f32(const float* const* grads, const long long* offs, const long long* ns,
                      int count, float* w, float* st0, float* st1, const ArenaOptHyper& h,
                      hipStream_t stream) {
  return mt_launch_groups(reinterpret_cast<const void* const*>(grads), offs, ns, count,
                          [&](const MtArgs& a, int blocks, int, int) {
    hipLaunchKernelGGL(mt_f32_kernel<RULE>, dim3(blocks), dim3(256), 0, stream, a, w, st0, st1, h);
    return hipGetLastError();
  });
}

// What a rule needs beyond its segments: its second state buffer, Adam its corr, Nesterov a
// momentum above 0.
inline bool rule_args_ok(int rule, const float* st0, const float* st1, const ArenaOptHyper& h) {
  if (rule != ARENA_OPT_SGD && rule != ARENA_OPT_RMSPROP && rule != ARENA_OPT_ADAM &&
      rule != ARENA_OPT_NESTEROV)
    return false;
  if (rule == ARENA_OPT_NESTEROV) return st0 && h.b > 0.f;
  return st0 && (rule == ARENA_OPT_SGD || st1) && (rule != ARENA_OPT_ADAM || h.corr);
}

template <class RULE>
hipError_t launch_shard(const void* grad, int grad_bf16, float* w32, float* st0, float* st1,
                        void* wbf, long long n, const ArenaOptHyper& h, hipStream_t stream) {
  const dim3 grid((unsigned)std::min<long long>((n + 1023) / 1024, 4096)), block(256);
  uint16_t* wb = reinterpret_cast<uint16_t*>(wbf);
  if (grad_bf16)
    hipLaunchKernelGGL((shard_update_kernel<RULE, SHARD_MASTER>), grid, block, 0, stream, grad, w32,
                       st0, st1, wb, n, h);
  else if (wbf)
    hipLaunchKernelGGL((shard_update_kernel<RULE, SHARD_WIDE>), grid, block, 0, stream, grad, w32,
                       st0, st1, wb, n, h);
  else
    hipLaunchKernelGGL((shard_update_kernel<RULE, SHARD_F32>), grid, block, 0, stream, grad, w32,
                       st0, st1, wb, n, h);
  return hipGetLastError();
}

// The pieces of a shard as the multi-tensor walk takes them: piece i's gradient pointer.
std::vector<const void*> piece_grads(const void* grad, int grad_bf16, const long long* goffs,
                                     int count) {
  std::vector<const void*> ptrs(count);
  for (int i = 0; i < count; ++i)
    ptrs[i] = reinterpret_cast<const char*>(grad) + goffs[i] * (grad_bf16 ? 2 : 4);
  return ptrs;
}

bool pieces_ok(const long long* goffs, const long long* moffs, const long long* ns,
               const int* slots, int count, int n_slots) {
  if (count < 0 || n_slots < 0 || !mt_segments_ok(goffs, ns, count, 4) ||
      !mt_segments_ok(moffs, ns, count, 4))
    return false;
  for (int i = 0; i < count; ++i)
    if (slots[i] < 0 || slots[i] >= n_slots) return false;
  return true;
}

}  // namespace

// =============================================================================================
// Host launchers (plain C ABI; the torch binding TU validates shapes before calling these).
// =============================================================================================
extern "C" {

hipError_t arena_adam_flat(float* P, float* M, float* V, const float* G, long long n,
                           ArenaAdam adam, ArenaCounterOp ctr, hipStream_t stream) {
  if (n % 4) return hipErrorInvalidValue;
  const long long n4 = n / 4;
  const int blocks = (int)std::min<long long>((n4 + 255) / 256, 2048);
  hipLaunchKernelGGL(adam_flat_kernel, dim3(blocks > 0 ? blocks : 1), dim3(256), 0, stream, P, M, V,
                     G, n4, adam, ctr);
  return hipGetLastError();
}

hipError_t arena_sgd_flat(float* P, const float* G, long long n, float lr, const float* lr_ptr,
                          float gscale, hipStream_t stream) {
  if (n % 4) return hipErrorInvalidValue;
  const long long n4 = n / 4;
  const int blocks = (int)std::min<long long>((n4 + 255) / 256, 2048);
  hipLaunchKernelGGL(sgd_flat_kernel, dim3(blocks > 0 ? blocks : 1), dim3(256), 0, stream, P, G, n4,
                     lr, lr_ptr, gscale);
  return hipGetLastError();
}

// ptrs/offs/ns arrays of length count (any count; chunked into launches of kMtMax tensors).
hipError_t arena_mt_copy_scale(float* const* ptrs, const long long* offs, const long long* ns,
                               int count, float* flat, float scale, int dir, hipStream_t stream) {
  if (!mt_segments_ok(offs, ns, count, 1)) return hipErrorInvalidValue;
  return mt_launch_groups(reinterpret_cast<const void* const*>(ptrs), offs, ns, count,
                          [&](const MtArgs& a, int blocks, int, int) {
    hipLaunchKernelGGL(mt_copy_scale_kernel, dim3(blocks), dim3(256), 0, stream, a, flat, scale,
                       dir);
    return hipGetLastError();
  });
}

// Master layout. grads[i]: bf16 gradient pointers; offs/ns: segment offsets and sizes, multiples
// of 4. st1: the rule's second state buffer (SGD, Nesterov: unused, may be null). hyper.scale is
// not read by SGD and Nesterov and is 1 for the others on this path, whatever the caller left in it.
hipError_t arena_mt_update_master(int rule, const void* const* grads, const long long* offs,
                                  const long long* ns, int count, float* master, float* st0,
                                  float* st1, void* wbf, ArenaOptHyper hyper, hipStream_t stream) {
  if (!rule_args_ok(rule, st0, st1, hyper) || !mt_segments_ok(offs, ns, count, 4))
    return hipErrorInvalidValue;
  hyper.scale = 1.f;
  if (rule == ARENA_OPT_SGD)
    return launch_master<SgdRule>(grads, offs, ns, count, master, st0, st1, wbf, hyper, stream);
  if (rule == ARENA_OPT_NESTEROV)
    return launch_master<NesterovRule>(grads, offs, ns, count, master, st0, st1, wbf, hyper, stream);
  if (rule == ARENA_OPT_RMSPROP)
    return launch_master<RmspropRule>(grads, offs, ns, count, master, st0, st1, wbf, hyper, stream);
  return launch_master<AdamRule>(grads, offs, ns, count, master, st0, st1, wbf, hyper, stream);
}

// fp32 layout. grads[i]: fp32 gradient pointers; offs/ns: segment offsets and sizes in w and the
// state buffers (any values). SGD here is SgdScaledRule: d = g * scale + wd * w; Nesterov is
// NesterovScaledRule.
hipError_t arena_mt_update_f32(int rule, const float* const* grads, const long long* offs,
                               const long long* ns, int count, float* w, float* st0, float* st1,
                               ArenaOptHyper hyper, hipStream_t stream) {
  if (!rule_args_ok(rule, st0, st1, hyper) || !mt_segments_ok(offs, ns, count, 1))
    return hipErrorInvalidValue;
  if (rule == ARENA_OPT_SGD)
    return launch_f32<SgdScaledRule>(grads, offs, ns, count, w, st0, st1, hyper, stream);
  if (rule == ARENA_OPT_NESTEROV)
    return launch_f32<NesterovScaledRule>(grads, offs, ns, count, w, st0, st1, hyper, stream);
  if (rule == ARENA_OPT_RMSPROP)
    return launch_f32<RmspropRule>(grads, offs, ns, count, w, st0, st1, hyper, stream);
  return launch_f32<AdamRule>(grads, offs, ns, count, w, st0, st1, hyper, stream);
}

hipError_t arena_shard_sgd(const void* grad, int grad_bf16, float* w32, float* mom, void* wbf,
                           long long n, float lr, const float* lr_ptr, float mu, float wd,
                           float scale, hipStream_t stream) {
  if (n % 4 || (grad_bf16 && !wbf)) return hipErrorInvalidValue;
  if (n == 0) return hipSuccess;
  const long long blocks = std::min<long long>((n + 1023) / 1024, 4096);
  if (grad_bf16)
    hipLaunchKernelGGL(shard_sgd_kernel<true>, dim3((unsigned)blocks), dim3(256), 0, stream, grad,
                       w32, mom, reinterpret_cast<uint16_t*>(wbf), n, lr, lr_ptr, mu, wd, scale);
  else
    hipLaunchKernelGGL(shard_sgd_kernel<false>, dim3((unsigned)blocks), dim3(256), 0, stream, grad,
                       w32, mom, nullptr, n, lr, lr_ptr, mu, wd, scale);
  return hipGetLastError();
}

// `rule` over one flat range (a rank's shard of a reduce-scattered bucket), n % 4 == 0:
//   grad_bf16, wbf:   bf16 gradient, fp32 master w32 and states, rounded bf16 weights to wbf
//   fp32 grad, !wbf:  the fp32 weights w32 are their own masters
//   fp32 grad, wbf:   the wide layout: fp32 gradient, fp32 master and states, bf16 weights to wbf
// RMSProp and Adam (st1, Adam: hyper.corr) and Nesterov SGD (NesterovScaledRule) in all three;
// SGD (SgdScaledRule) in the wide layout only: the other two are arena_shard_sgd's, whose bits
// must not move.
hipError_t arena_shard_update(int rule, const void* grad, int grad_bf16, float* w32, float* st0,
                              float* st1, void* wbf, long long n, ArenaOptHyper hyper,
                              hipStream_t stream) {
  if (!grad || !w32 || n < 0 || n % 4 || (grad_bf16 && !wbf) ||
      !rule_args_ok(rule, st0, st1, hyper) || (rule == ARENA_OPT_SGD && (grad_bf16 || !wbf)))
    return hipErrorInvalidValue;
  if (n == 0) return hipSuccess;
  if (rule == ARENA_OPT_SGD)
    return launch_shard<SgdScaledRule>(grad, grad_bf16, w32, st0, st1, wbf, n, hyper, stream);
  if (rule == ARENA_OPT_NESTEROV)
    return launch_shard<NesterovScaledRule>(grad, grad_bf16, w32, st0, st1, wbf, n, hyper, stream);
  if (rule == ARENA_OPT_RMSPROP)
    return launch_shard<RmspropRule>(grad, grad_bf16, w32, st0, st1, wbf, n, hyper, stream);
  return launch_shard<AdamRule>(grad, grad_bf16, w32, st0, st1, wbf, n, hyper, stream);
}

// Sharded LARS, first half: sums[2 * s] / sums[2 * s + 1] = this rank's fp64 sums of w^2 / (g *
// scale)^2 over the piece of tensor s (0.0 for the tensors without one); n_slots tensors. Piece i:
// ns[i] elements at grad + goffs[i] and master + moffs[i] (multiples of 4), slots[i] distinct.
// workspace: arena_mt_lars_workspace_floats(ns, count) floats, as arena_mt_lars_master's.
hipError_t arena_shard_lars_norms(const void* grad, int grad_bf16, const long long* goffs,
                                  const long long* moffs, const long long* ns, const int* slots,
                                  int count, int n_slots, const float* master, float scale,
                                  float* workspace, double* sums, hipStream_t stream) {
  if (!sums || !pieces_ok(goffs, moffs, ns, slots, count, n_slots) ||
      (count > 0 && (!grad || !master || !workspace)))
    return hipErrorInvalidValue;
  if (n_slots == 0) return hipSuccess;
  hipLaunchKernelGGL(f64_zero_kernel, dim3((2 * n_slots + 255) / 256), dim3(256), 0, stream, sums,
                     2 * n_slots);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  const std::vector<const void*> ptrs = piece_grads(grad, grad_bf16, goffs, count);
  float2* part = reinterpret_cast<float2*>(workspace);
  int part_base = 0;
  return mt_launch_groups(ptrs.data(), moffs, ns, count,
                          [&](const MtArgs& a, int blocks, int base, int cnt) {
    LarsSlots s;
    for (int i = 0; i < kMtMax; ++i) s.slot[i] = i < cnt ? slots[base + i] : 0;
    s.part_base = part_base;
    part_base += blocks;
    const dim3 grid((blocks + 3) / 4), block(256);
    if (grad_bf16)
      hipLaunchKernelGGL(shard_lars_part_kernel<false>, grid, block, 0, stream, a, s.part_base,
                         master, scale, part);
    else
      hipLaunchKernelGGL(shard_lars_part_kernel<true>, grid, block, 0, stream, a, s.part_base,
                         master, scale, part);
    const hipError_t e2 = hipGetLastError();
    if (e2 != hipSuccess) return e2;
    hipLaunchKernelGGL(shard_lars_sums_kernel, dim3(cnt), block, 0, stream, a, s, part, sums);
    return hipGetLastError();
  });
}

// Sharded LARS, second half, after the all-reduce of sums: trust[s] for all n_slots tensors, and
// momentum SGD (SgdScaledRule) with step lr * trust over this rank's pieces. hyper: ArenaOptHyper's
// LARS column and scale.
hipError_t arena_shard_lars_update(const void* grad, int grad_bf16, const long long* goffs,
                                   const long long* moffs, const long long* ns, const int* slots,
                                   int count, int n_slots, float* master, float* mom, void* wbf,
                                   const double* sums, float* trust, ArenaOptHyper hyper,
                                   hipStream_t stream) {
  if (!trust || !sums || !(hyper.a > 0.f) || !(hyper.eps >= 0.f) ||
      !pieces_ok(goffs, moffs, ns, slots, count, n_slots) ||
      (count > 0 && (!grad || !master || !mom || !wbf)))
    return hipErrorInvalidValue;
  if (n_slots == 0) return hipSuccess;
  hipLaunchKernelGGL(shard_lars_trust_kernel, dim3((n_slots + 255) / 256), dim3(256), 0, stream,
                     sums, trust, n_slots, hyper);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  const std::vector<const void*> ptrs = piece_grads(grad, grad_bf16, goffs, count);
  return mt_launch_groups(ptrs.data(), moffs, ns, count,
                          [&](const MtArgs& a, int blocks, int base, int cnt) {
    LarsSlots s;
    for (int i = 0; i < kMtMax; ++i) s.slot[i] = i < cnt ? slots[base + i] : 0;
    s.part_base = 0;
    uint16_t* wb = reinterpret_cast<uint16_t*>(wbf);
    if (grad_bf16)
      hipLaunchKernelGGL(shard_lars_update_kernel<false>, dim3(blocks), dim3(256), 0, stream, a, s,
                         master, mom, wb, sums, hyper);
    else
      hipLaunchKernelGGL(shard_lars_update_kernel<true>, dim3(blocks), dim3(256), 0, stream, a, s,
                         master, mom, wb, sums, hyper);
    return hipGetLastError();
  });
}

hipError_t arena_lr_schedule(const long long* seg, int n_seg, long long* step, float* lr,
                             hipStream_t stream) {
  if (n_seg < 1 || n_seg > 64) return hipErrorInvalidValue;
  hipLaunchKernelGGL(lr_schedule_kernel, dim3(1), dim3(1), 0, stream, seg, n_seg, step, lr);
  return hipGetLastError();
}

long long arena_mt_lars_workspace_floats(const long long* ns, int count) {
  long long blocks = 0;
  for (int i = 0; i < count; ++i) blocks += (ns[i] + 1023) / 1024;
  return 2 * blocks;
}

// LARS over bf16 gradients with fp32 masters: offs / ns multiples of 4, as arena_mt_update_master.
// slots[i]: tensor i's entry of trust. workspace: arena_mt_lars_workspace_floats(ns, count) floats,
// 16-byte aligned, contents irrelevant: one (w^2, g^2) pair per 1024-element block, each launch
// group in its own range. hyper: ArenaOptHyper's LARS column.
hipError_t arena_mt_lars_master(const void* const* grads, const long long* offs,
                                const long long* ns, const int* slots, int count, float* master,
                                float* mom, void* wbf, float* trust, float* workspace,
                                ArenaOptHyper hyper, hipStream_t stream) {
  if (!trust || !workspace || !(hyper.a > 0.f) || !(hyper.eps >= 0.f) ||
      !mt_segments_ok(offs, ns, count, 4))
    return hipErrorInvalidValue;
  for (int i = 0; i < count; ++i)
    if (slots[i] < 0) return hipErrorInvalidValue;
  float2* part = reinterpret_cast<float2*>(workspace);
  int part_base = 0;
  return mt_launch_groups(grads, offs, ns, count,
                          [&](const MtArgs& a, int blocks, int base, int cnt) {
    LarsSlots s;
    for (int i = 0; i < kMtMax; ++i) s.slot[i] = i < cnt ? slots[base + i] : 0;
    s.part_base = part_base;
    part_base += blocks;
    hipLaunchKernelGGL(mt_lars_norms_kernel, dim3((blocks + 3) / 4), dim3(256), 0, stream, a, s,
                       master, part);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(mt_lars_update_kernel, dim3(blocks), dim3(256), 0, stream, a, s, master,
                       mom, reinterpret_cast<uint16_t*>(wbf), part, trust, hyper);
    return hipGetLastError();
  });
}

hipError_t arena_adam_tick(long long* step, double* pw, float* corr, double b1, double b2,
                           hipStream_t stream) {
  hipLaunchKernelGGL(adam_tick_kernel, dim3(1), dim3(1), 0, stream, step, pw, corr, b1, b2);
  return hipGetLastError();
}

}  // extern "C"
