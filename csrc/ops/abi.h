// Plain-C ABI shared by the HIP kernel TUs and the host binding TU (no device code here).
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <hip/hip_runtime_api.h>

// BatchNorm statistics accumulators ("acc mode", bn_kernels.hip / conv_kernels.hip): every fp64
// set is ARENA_ACC_REP consecutive [2][C] replicas; a consumer sums all of them, in replica order.
// The conv epilogues (up to 3136 tiles per channel at batch 128) add row tile mt's sums into
// replica mt % ARENA_ACC_REP, so their same-address fp64 atomics do not serialize; the BN passes'
// reductions (at most 512 block sums per channel) add into replica 0.
#define ARENA_ACC_REP 4

// Convolution variant codes (stable: the autotuner stores them in plans and plan files). Every
// kernel form is ONE row of a table in conv_kernels.hip (kFwdRows / kWgradRows), from which its
// launch is instantiated; arena_conv_variant / arena_conv_wgrad_variant return a row and
// arena_conv_variants / arena_conv_wgrad_variants every code. arena_amd/ops/conv_variants.py holds
// the planner's copy of the rows; tests/test_conv.py compares the two field by field.
// Forward / backward-data codes: a row's code, and for a row that may be split
//   code + ARENA_CONV_SPLIT_STRIDE * (ks - 1): the same tile with its K steps split over
//   ks <= ARENA_CONV_SPLIT_STRIDE blocks.
#define ARENA_CONV_SPLIT_STRIDE 16

// ----------------------------------------------------------------------------------------------
// Host-visible plain-C ABI structs shared with the torch binding TU (bindings.cpp).
// ----------------------------------------------------------------------------------------------
extern "C" {

// Where the rows of an A operand (or the labels) come from. Row r of the logical batch is
//   phys = idx ? idx[((*cursor + cursor_off) * batch + r) % idx_len] : r
// which fuses the data-loader gather (dataset permutation + per-step cursor) into the GEMM.
struct ArenaRowSource {
  const void* ptr;
  int dtype;            // 0 = f32, 1 = u8, 2 = i32, 3 = i64
  int ld;               // row stride in elements
  float scale;          // multiplied on load (1/255 for u8 pixels)
  const int* idx;       // optional gather permutation (device)
  long long idx_len;
  const long long* cursor;  // optional device counter (completed steps)
  int cursor_off;       // added to *cursor (lets a kernel read the step counter it does not commit)
  int batch;            // rows consumed per cursor step
};

// Device step counters: dst = (src ? *src : 0) + add, executed by one lane of block 0.
struct ArenaCounterOp {
  long long* dst;
  const long long* src;
  int add;
};

struct ArenaAdam {
  float lr;               // used when lr_ptr == nullptr
  const float* lr_ptr;    // optional device learning rate (schedules under graph replay)
  float beta1, beta2, eps, weight_decay;
  const long long* t_ptr; // device Adam step t (1-based) for bias correction
  float grad_scale;       // e.g. 1/world_size for averaged all-reduce gradients
  int tf_style;           // 1: TF AdamOptimizer epsilon placement, 0: torch.optim.Adam
};

// The multi-tensor optimizer updates (csrc/ops/optim_kernels.hip): which rule, and its numbers.
// RMSProp and Adam are TF1's forms (arena_amd/ops/reference.py defines them); 1 - rho / 1 - b1 /
// 1 - b2 are formed in fp64 by the caller: the fp32 difference 1 - float(0.999) is 4.7e-5 off.
enum { ARENA_OPT_SGD = 0, ARENA_OPT_RMSPROP = 1, ARENA_OPT_ADAM = 2, ARENA_OPT_NESTEROV = 3 };
struct ArenaOptHyper {
  float lr;             // replaced by *lr_ptr when that is set
  const float* lr_ptr;  // device learning rate (DeviceLR), or null
  const float* corr;    // Adam: the clock's sqrt(1 - b2^t) / (1 - b1^t); the others: null
  float a, oma;         // RMSProp: rho, 1 - rho;  Adam: b1, 1 - b1;  LARS: eeta, unused
  float b, omb;         // SGD, Nesterov, LARS, RMSProp: momentum, unused;  Adam: b2, 1 - b2
  float eps, wd;        // RMSProp, Adam, LARS: their epsilon (SGD: unused); weight decay
  float scale;          // gradient scale (fp32 layout and shard_sgd; the master layout has none)
};

// One layer of a grouped weight-gradient launch (wgrad_grouped).
struct ArenaWGradProblem {
  ArenaRowSource x;       // rows m of the layer input
  int xt;                 // 0 f32, 1 u8
  const float* dz;        // [M][N] upstream gradient (null when derived from the softmax head)
  // Softmax-head modes (fused MLP step, see ArenaHead):
  //   hd_mode 1: dz = dlogits                               (output layer, N == C)
  //   hd_mode 2: dz = (dlogits · hd_w2) ⊙ (hd_h > 0) / keep  (hidden layer: ReLU+dropout bwd)
  int hd_mode;
  const float* hd_w2;     // [C][N] W2 snapshot (mode 2)
  const float* hd_h;      // [M][N] post-dropout activation, mask source (mode 2)
  float hd_inv_keep;
  int M, K, N;
  int mode;               // 0: write grad (scaled), 1: Adam in place
  float* gW; float* gB;   // mode 0 outputs ([N][K], [N]); gB may be null
  float* pW; float* mW; float* vW;  // mode 1
  float* pB; float* mB; float* vB;
  int tiles_k, tiles_n, block_begin;
  int x_par_stride;       // bytes between the two halves of a step-parity double buffer: the rows
                          // come from half (step & 1) of x (head modes only); 0: x is one buffer
};

// Softmax-cross-entropy head recomputed inside every wgrad workgroup from the raw logits that the
// forward kernel accumulated (100 x 10 for MNIST: cheaper than any inter-workgroup hand-off).
// logits2 is double-buffered by step parity: step t accumulates into buffer t&1 while the wgrad
// of step t zeroes buffer (t+1)&1 for the next forward.
struct ArenaHead {
  float* logits2;           // [2][M][C] Σ over hidden tiles of H·W2ᵀ (no bias)
  const long long* step;    // device step counter: (*step + step_off) = index of this step
  int step_off;
  int parity;               // -1: buffer (*step + step_off) & 1; 0/1: known at launch, so the
                            // logits loads need not wait for the step counter
  const float* b2;          // [C]
  int C;
  ArenaRowSource lab;       // labels (same gather as the layer input)
  float loss_scale;         // 1/batch (mean loss)
  int lab_par_stride;       // labels between the halves of a step-parity double buffer, 0: none
  float* loss_acc; int* correct_acc; int hist_len;  // metric ring (block 0), power of two
  // optional (batch ahead): extra workgroups of the launch copy the NEXT step's batch, the u8 rows
  // na_x[p][0 .. na_K) and labels na_lab[p] of p = na_perm[((step + 1) * na_batch + r) % na_len],
  // into half (step + 1) & 1 of na_xa [2][na_batch][na_K] / na_ya [2][na_batch], so the next
  // forward loads its X rows from an address it knows at launch
  const int* na_perm; long long na_len; int na_batch;
  const uint8_t* na_x; int na_ld, na_K;
  const void* na_lab; int na_lab_dtype;   // dtype codes of ArenaRowSource
  uint8_t* na_xa; int* na_ya;
};


// Fused training BatchNorm (csrc/ops/bn_kernels.hip). Per-channel fp32 arrays of length C.
struct ArenaBNStats {
  float eps, momentum;
  const float* gamma;     // optional (affine off -> 1)
  const float* beta;      // optional (-> 0)
  float* mean;            // out (training) / in (eval: running mean): batch mean
  float* invstd;          // out: 1 / sqrt(biased var + eps)
  float* scale;           // out (training) / in (eval): gamma * invstd
  float* shift;           // out (training) / in (eval): beta;  y = (x - mean) * scale + shift
  float* running_mean;    // optional, updated in place with momentum (unbiased variance)
  float* running_var;
  long long* batches;     // optional nn.BatchNorm num_batches_tracked, += 1 by the finalize kernel
};

struct ArenaBNBwd {
  const float* mean;      // saved batch statistics of the forward
  const float* invstd;
  const float* gamma;     // optional
  float* dgamma;          // optional outputs
  float* dbeta;
  float* ca; float* cb; float* cc;  // workspace [C] each: dx = ca * (g - cb - (x - mean) * cc)
  // the forward's y = act((x - mean) * scale + shift): the fused stem (BN + ReLU + max pool,
  // arena_bn_pool_bwd) recomputes its ReLU mask from x with them
  const float* scale; const float* shift;
};

// One forward / backward-data convolution variant (see ARENA_CONV_SPLIT_STRIDE above).
enum {
  ARENA_CONV_V1 = 0,        // 16x16x32 MFMAs on 4 waves (conv_fwd_kernel / conv_wgrad_kernel)
  ARENA_CONV_V1_W8 = 1,     // the same body on 8 waves, 256-row tiles (conv_fwd_kernel_w8)
  ARENA_CONV_V2 = 2,        // 32x32x16 MFMAs, LDS epilogue (conv2_kernel / conv_wgrad2_kernel)
  ARENA_CONV_V2_OCC4 = 3,   // its serial single-buffer form, four waves per SIMD
  ARENA_CONV_V2_HALO = 4    // its 3x3 / stride 1 / pad 1 halo form (conv2_kernel_halo)
};
struct ArenaConvVariant {
  int code, base;         // base: the unsplit code of the same tile (== code when ksplit == 1)
  int bm, bn;             // output tile: pixels x channels
  int family;             // ARENA_CONV_V1 ...
  int nwm, nwn, nbuf;     // waves along bm / bn; stage buffers (halo: weight ring buffers)
  int ksplit;             // split-K factor of this code
  int max_width;          // halo: the widest image its window holds; 0: no limit
  int even_chunks;        // two wave groups split the 64-channel chunks: C / 64 must be even
  int wide8;              // an 8-wave halo form
  int c16, phases;        // has a c16 (stem) form; runs strided-dgrad phases in one launch
  int may_split;          // the codes base + ARENA_CONV_SPLIT_STRIDE * (ks - 1) exist
};

// One weight-gradient variant: a bm x bn (Cout x R*S*C) tile. family: ARENA_CONV_V1 or _V2.
struct ArenaConvWgradVariant {
  int code, bm, bn, family;
  int nwm, nwn, nbuf;
  int serial;             // single stage buffer, four waves per SIMD
  int groups;             // wave groups per block that split its pixel steps
  int c16;
};

// One batch of the device-resident image pipeline (csrc/ops/data_kernels.hip).
struct ArenaImageBatch {
  const uint8_t* images;    // [n][S][S][3] uint8
  const long long* labels;  // [n]
  long long n;
  const int* perm;          // [L] dataset rows, each in [0, n)
  long long L;
  long long* cursor;        // device counter of completed batches (read; += 1 when advancing)
  const void* table;        // [3][256] normalised values in the output dtype
  void* out;                // z [B][Hc/2][Wc/2][16] bf16, or x [B][Hc][Wc][3] bf16 / fp32
  long long* labels_out;    // [B]
  int* rows_out;            // [B]
  int* crop_out;            // [B][3]: y0, x0, flip
  int S, B, Hc, Wc;
  int train;                // 1: shuffled rows (wrapping), random crop + flip; 0: in order,
                            // centre crop, rows past L are padding
  uint32_t seed;
  int stream;               // draw stream (the data-parallel rank)
};

// The colour distortion of arena_image_batch_color (semantics: ops/reference.py image_batch_color).
struct ArenaImageColor {
  const int* matrices;      // [n_matrices][9]: candidate 3 x 3 colour maps in 1/4096ths, row-major
  int n_matrices;           // 1 .. 4096
  int k_lo, k_hi;           // contrast range in 1/256ths, 0 <= k_lo <= k_hi <= 4096
  int delta;                // largest |brightness| in bytes, 0 .. 255
  int* sums;                // [B][blocks per image][3]: each block's channel sums (scratch;
                            // blocks per image = ceil((Hc / 2) (Wc / 2) / 256))
  int* color_out;           // [B][3]: matrix index, contrast, brightness
};

// Intra-node xGMI collective (csrc/ccl/xgmi_ccl.hip): every rank's registered buffers, mapped into
// this process through hipIpc handles (buf[rank] / sig[rank] are the local allocations).
#define ARENA_CCL_MAX_RANKS 8
#define ARENA_CCL_MAX_BLOCKS 256
// One-shot allreduce region: 2 x ONESHOT_ELEMS floats (double-buffered by call parity) that sit
// right after the buf_elems floats of every staging buffer (the host allocates them).
#define ARENA_CCL_ONESHOT_ELEMS 16384
// barrier phases per call (the scatter + all-gather broadcast uses three)
#define ARENA_CCL_PHASES 3
struct ArenaXgmiPeers {
  float* buf[ARENA_CCL_MAX_RANKS];    // staging / gradient buffer of each rank (+ one-shot tail)
  float* buf2[ARENA_CCL_MAX_RANKS];   // second buffer (parameters for the fused Adam step)
  uint32_t* sig[ARENA_CCL_MAX_RANKS]; // uncached flags: [3 phases][MAX_BLOCKS][MAX_RANKS]
  uint32_t* epoch;                    // local, per block: calls completed
  int* err;                           // local: set to 1 when a barrier wait timed out
  long long buf_elems;                // capacity of buf[] (floats)
  long long buf2_elems;
  int rank, world;
  // 0 (default): every kernel stores only into this rank's own buffers and peers PULL the owner's
  // chunk after a barrier; 1: the owner pushes its chunk into every peer's buffer (one barrier
  // less for the two-shot allreduce; used only when its own construction-time self-test passed)
  int push;
  long long timeout_cycles;           // barrier wait bound in s_memrealtime ticks (100 MHz)
};

// ----------------------------------------------------------------------------------------------
// Every host-callable launcher, declared once: each .hip unit includes this header ahead of its
// definitions (a mismatch is a "conflicting types" compile error there) and bindings.cpp calls
// through it. Names only -- what the arguments mean is documented at the definitions.
// ----------------------------------------------------------------------------------------------
// csrc/ops/mlp_kernels.hip
hipError_t arena_linear_fwd(ArenaRowSource src, const float* W, const float* bias, float* Y, int M,
                            int N, int K, int act, float keep_prob, uint32_t seed,
                            const long long* step_src, hipStream_t stream);
hipError_t arena_mlp_fwd_logits(ArenaRowSource src, const float* W, const float* bias, float* Y,
                                int M, int N, int K, float keep_prob, uint32_t seed,
                                const long long* step_src, const float* W2, float* W2_copy, int C,
                                float* logits2, uint8_t* xb, const void* lab_ptr, int lab_dtype,
                                int* yb, ArenaCounterOp ctr, const uint8_t* xa, int xa_parity,
                                hipStream_t stream);
hipError_t arena_xent_head(const float* H, int M, int D, const float* W2, const float* b2, int C,
                           ArenaRowSource lab, float* dlogits, float* dZ, float keep_prob,
                           int relu_mask, float loss_scale, float* loss_acc, int* correct_acc,
                           int hist_len, const long long* hist_step, ArenaCounterOp ctr,
                           hipStream_t stream);
hipError_t arena_wgrad_grouped(ArenaWGradProblem* probs, int nprob, ArenaAdam adam,
                               float grad_scale, ArenaCounterOp ctr, ArenaHead head,
                               hipStream_t stream);
void arena_wgrad_short_images(int on);
void arena_mlp_static_step(int on);
int arena_mlp_static_step_last(int which);  // 0: forward, 1: backward; 1 = static instantiation
hipError_t arena_softmax_xent(const float* logits, const long long* labels, int M, int C,
                              float* loss, float* dlogits, float grad_scale, hipStream_t stream);
#ifdef ARENA_TIMELINE
hipError_t arena_timeline_read(long long* host, int clear);
#endif

// csrc/ops/optim_kernels.hip
hipError_t arena_adam_flat(float* P, float* M, float* V, const float* G, long long n,
                           ArenaAdam adam, ArenaCounterOp ctr, hipStream_t stream);
hipError_t arena_sgd_flat(float* P, const float* G, long long n, float lr, const float* lr_ptr,
                          float gscale, hipStream_t stream);
hipError_t arena_mt_copy_scale(float* const* ptrs, const long long* offs, const long long* ns,
                               int count, float* flat, float scale, int dir, hipStream_t stream);
// Multi-tensor updates by `rule` (ARENA_OPT_*, hyper: ArenaOptHyper's column for it), one launch
// per 48 tensors; gradient i updates [offs[i], offs[i] + ns[i]) of the flat buffers. st0 / st1: the
// rule's fp32 state buffers (SGD and Nesterov SGD keep one: st1 is not touched; Nesterov needs a
// momentum above 0).
//   _master: bf16 gradients, fp32 masters and states, rounded bf16 weights to wbf (offs / ns
//            multiples of 4); no gradient scale.
//   _f32:    fp32 tensors and gradients, any sizes and offsets.
hipError_t arena_mt_update_master(int rule, const void* const* grads, const long long* offs,
                                  const long long* ns, int count, float* master, float* st0,
                                  float* st1, void* wbf, ArenaOptHyper hyper, hipStream_t stream);
hipError_t arena_mt_update_f32(int rule, const float* const* grads, const long long* offs,
                               const long long* ns, int count, float* w, float* st0, float* st1,
                               ArenaOptHyper hyper, hipStream_t stream);
hipError_t arena_shard_sgd(const void* grad, int grad_bf16, float* w32, float* mom, void* wbf,
                           long long n, float lr, const float* lr_ptr, float mu, float wd,
                           float scale, hipStream_t stream);
// `rule` over one flat range (a data-parallel rank's shard), n % 4 == 0, pointers aligned as for
// arena_shard_sgd, grid-stride with the same 4096-block cap. Layouts: bf16 grad + wbf (fp32 master,
// bf16 weights written); fp32 grad without wbf (fp32 weights are their own masters); fp32 grad +
// wbf (wide: fp32 master, bf16 weights written). RMSProp / Adam (st1; Adam: hyper.corr) and
// Nesterov SGD (st1 unused) in all three, SGD (st1 unused) in the wide layout only; anything else
// is hipErrorInvalidValue.
hipError_t arena_shard_update(int rule, const void* grad, int grad_bf16, float* w32, float* st0,
                              float* st1, void* wbf /*nullable*/, long long n, ArenaOptHyper hyper,
                              hipStream_t stream);
// Sharded LARS. A shard's pieces: piece i is ns[i] elements (a multiple of 4) at grad + goffs[i]
// (bf16 or fp32 summed gradient) and master + moffs[i], of tensor slots[i] in [0, n_slots).
//   _norms:  sums[2 s] / sums[2 s + 1] = fp64 sums of w^2 / (g * scale)^2 over this rank's piece of
//            tensor s, 0.0 without one (all 2 * n_slots written; no atomics, fixed order).
//            workspace: arena_mt_lars_workspace_floats(ns, count) floats, never read before written.
//   -- the caller all-reduces sums (SUM) over the ranks that share the tensors --
//   _update: trust[s] for every s from the reduced sums (as arena_mt_lars_master forms it), then
//            d = g * scale + wd * w; m = mu * m + d; w -= lr * trust * m over the pieces, rounded
//            bf16 weights to wbf. hyper: the LARS column and scale.
hipError_t arena_shard_lars_norms(const void* grad, int grad_bf16, const long long* goffs,
                                  const long long* moffs, const long long* ns, const int* slots,
                                  int count, int n_slots, const float* master, float scale,
                                  float* workspace, double* sums, hipStream_t stream);
hipError_t arena_shard_lars_update(const void* grad, int grad_bf16, const long long* goffs,
                                   const long long* moffs, const long long* ns, const int* slots,
                                   int count, int n_slots, float* master, float* mom, void* wbf,
                                   const double* sums, float* trust, ArenaOptHyper hyper,
                                   hipStream_t stream);
// lr[0] = value of the piecewise-linear schedule seg[n_seg][4] (begin, end, lr0 bits, lr1 bits;
// fp64 values as int64 bit patterns) at *step, then *step += 1.
hipError_t arena_lr_schedule(const long long* seg, int n_seg, long long* step, float* lr,
                             hipStream_t stream);
// LARS (arena_amd/ops/reference.py) over bf16 gradients with fp32 masters, two launches per 48
// tensors: per-block partial sums of w^2 and g^2 into workspace, then the update, whose blocks
// each reduce their tensor's partials, form trust = eeta * |w| / (|g| + wd * |w| + eps) (1 when a
// norm is 0) and step with lr * trust. trust[slots[i]] receives tensor i's ratio. workspace:
// arena_mt_lars_workspace_floats(ns, count) floats, 16-byte aligned, never read before written.
long long arena_mt_lars_workspace_floats(const long long* ns, int count);
hipError_t arena_mt_lars_master(const void* const* grads, const long long* offs,
                                const long long* ns, const int* slots, int count, float* master,
                                float* mom, void* wbf, float* trust, float* workspace,
                                ArenaOptHyper hyper, hipStream_t stream);
// t = *step + 1; pw[0] *= b1; pw[1] *= b2; *corr = float(sqrt(1 - pw[1]) / (1 - pw[0])) in fp64,
// every operation rounded on its own; *step = t.
hipError_t arena_adam_tick(long long* step, double* pw, float* corr, double b1, double b2,
                           hipStream_t stream);

// csrc/ops/bn_kernels.hip
void arena_bn_set_fin_max_blocks(int p);
void arena_bn_set_nt(int on);
void arena_bn_set_elem_max_blocks(int b);
void arena_bn_set_dx_max_blocks(int b);
void arena_bn_set_slice(int on);
void arena_bn_set_pool_quad_mult(int m);
void arena_bn_set_acc_max_pairs(long long p);
long long arena_bn_acc_max_pairs();
int arena_bn_acc_ok(long long M, int C);
// read-only views of the host-side path selection (tests assert the path a shape takes):
// row blocks of a reduction over M x C and their rows per block (0 for an unsupported shape);
// level-1 finalize blocks per channel group for nblk partials
long long arena_bn_reduce_blocks(long long M, int C, long long* rpb);
int arena_bn_fin_blocks(long long nblk);
void arena_bn_set_reduce_geometry(long long max_blocks, long long min_rounds);
long long arena_bn_lvl2_doubles(long long nblk, int C);
long long arena_bn_workspace_floats(long long M, int C);
hipError_t arena_bn_fwd(int dtype, const void* x, const void* res, void* y, uint8_t* mask,
                        long long M, int C, int relu, int training, float* part, int ext_nblk,
                        long long ext_rpb, double* lvl2, unsigned* tickets, ArenaBNStats st,
                        double* acc, int acc_ready, double* zero, int nzero, hipStream_t stream);
hipError_t arena_bn_bwd(int dtype, const void* dy, const uint8_t* mask, const void* x, void* dx,
                        void* dres, long long M, int C, int relu, float* part, int ext_nblk,
                        double* lvl2, unsigned* tickets, ArenaBNBwd co, double* acc, int fin_dx,
                        double* zero, int nzero, const void* x2, const float* mean2,
                        double* acc2, hipStream_t stream);
hipError_t arena_bn_pool_fwd(int dtype, const void* x, void* y, uint8_t* pos, void* xsel, int N,
                             int H, int W, int C, int k, int s, int p, ArenaBNStats st,
                             const double* fin, const float* part, int ext_nblk, long long ext_rpb,
                             double* lvl2, unsigned* tickets, double* zero, int nzero,
                             hipStream_t stream);
hipError_t arena_bn_pool_bwd(int dtype, const void* dy, const uint8_t* pos, const void* x,
                             const void* xsel, void* dx, int N, int H, int W, int C, int k, int s,
                             int p, ArenaBNBwd co, double* acc, double* zero, int nzero,
                             hipStream_t stream);

// csrc/ops/pool_kernels.hip
hipError_t arena_maxpool_fwd(int dtype, const void* x, void* y, uint8_t* pos, int N, int H, int W,
                             int C, int k, int s, int p, hipStream_t stream);
hipError_t arena_maxpool_bwd(int dtype, const void* dy, const uint8_t* pos, void* dx, int N, int H,
                             int W, int C, int k, int s, int p, hipStream_t stream);
hipError_t arena_xent_fwd(int dtype, const void* x, const long long* y, float* rowloss,
                          float* lse, int rows, int classes, hipStream_t stream);
hipError_t arena_xent_bwd(int dtype, const void* x, const long long* y, const float* lse,
                          const float* gout, void* dx, int rows, int classes, hipStream_t stream);
hipError_t arena_xent_ex_fwd(int dtype, const void* x, const long long* y, float* rowloss,
                             float* lse, int* meta, int rows, int classes, int has_ignore,
                             long long ignore_index, float eps, hipStream_t stream);
hipError_t arena_xent_ex_finalize(const float* rowloss, const int* meta, int rows, float* loss,
                                  float* inv_kept, long long* stats, hipStream_t stream);
hipError_t arena_xent_ex_bwd(int dtype, const void* x, const long long* y, const float* lse,
                             const int* meta, const float* inv_kept, const float* gout, void* dx,
                             int rows, int classes, float eps, hipStream_t stream);
hipError_t arena_gap_bwd(int dtype, const void* g, void* dx, int N, int HW, int C, float scale,
                         hipStream_t stream);

// csrc/ops/conv_kernels.hip
void arena_conv_set_stats_one_pass(int on);
void arena_conv_set_dbg(int bits);
hipError_t arena_conv_fwd_ex(const void* x, const void* w, void* y, float* part, const void* add,
                             const uint8_t* addmask, const void* bnx, const uint8_t* bnmask,
                             const float* bnmean, int N, int H, int W, int C, int Cout, int R,
                             int S, int stride, int pad_h, int pad_w, int Ho, int Wo,
                             const int* y_map, int c16, int variant, double* bn_acc, int ksplit,
                             void* kws, unsigned* kcnt, hipStream_t st);
hipError_t arena_conv_fwd_phases(const void* x, void* y, const void* add, int N, int H, int W,
                                 int C, int Cout, int Hy, int Wy, int osh, int osw, int nph,
                                 const void* const* w, const int* R, const int* S,
                                 const int* pad_h, const int* pad_w, const int* Ho, const int* Wo,
                                 const int* ooh, const int* oow, int variant, hipStream_t st);
int arena_conv_variant(int code, ArenaConvVariant* out);
int arena_conv_variants(int* codes, int cap);
hipError_t arena_conv_flip_multi(int n, const void* const* src, void* const* dst, const int* cout,
                                 const int* cin, const int* rs, hipStream_t st);
hipError_t arena_conv_phase_weights(const void* w, void* wt, int Cout, int C, int R, int S,
                                    int stride, int pad, long long* total, hipStream_t st);
hipError_t arena_conv_flip_weight(const void* w, void* wt, int Cout, int C, int R, int S,
                                  hipStream_t st);
hipError_t arena_s2d_stem(const void* x, void* z, int N, int H, int W, int C, int in_f32,
                          hipStream_t st);
hipError_t arena_stem_weight(const void* w, void* w16, int Cout, int C, long long sco,
                             long long sc, long long sr, long long ss, int w_f32, hipStream_t st);
hipError_t arena_stem_weight_grad(const void* dw16, void* dw, int Cout, int C, long long dco,
                                  long long dc, long long dr, long long ds, int dw_f32,
                                  hipStream_t st);
int arena_conv_wgrad_variant(int code, ArenaConvWgradVariant* out);
int arena_conv_wgrad_variants(int* codes, int cap);
int arena_conv_wgrad_splits(int N, int Ho, int Wo, int Cout, int Ktot, int variant,
                            int splits_hint);
hipError_t arena_conv_wgrad_ex(const void* x, const void* dy, float* ws, void* dw_bf16,
                               float* dw_f32, int N, int H, int W, int C, int Cout, int R, int S,
                               int stride, int pad_h, int pad_w, int Ho, int Wo, int c16,
                               int variant, int splits_hint, float scale, hipStream_t st);

// csrc/ops/data_kernels.hip
hipError_t arena_image_batch(ArenaImageBatch a, int layout, int out_f32, int advance,
                             hipStream_t st);
hipError_t arena_image_batch_resized(ArenaImageBatch a, const int* boxes, int n_boxes,
                                     int* box_out, int layout, int out_f32, int advance,
                                     hipStream_t st);
hipError_t arena_image_batch_color(ArenaImageBatch a, const int* boxes, int n_boxes, int* box_out,
                                   ArenaImageColor col, int layout, int out_f32, int advance,
                                   hipStream_t st);

// csrc/ccl/xgmi_ccl.hip
hipError_t arena_ccl_malloc(void** p, size_t bytes, int uncached);
hipError_t arena_ccl_free(void* p);
hipError_t arena_ccl_memset(void* p, int v, size_t bytes);
hipError_t arena_ccl_ipc_get(void* p, void* handle);
hipError_t arena_ccl_ipc_open(const void* handle, void** p);
hipError_t arena_ccl_ipc_close(void* p);
hipError_t arena_ccl_allreduce(const ArenaXgmiPeers* P, const float* in, float* out, long long n,
                               float scale, hipStream_t stream);
void arena_ccl_set_oneshot_max(long long e);
long long arena_ccl_get_oneshot_max();
hipError_t arena_ccl_adam(const ArenaXgmiPeers* P, float* M, float* V, long long n, ArenaAdam a,
                          ArenaCounterOp ctr, hipStream_t stream);
void arena_ccl_set_block_elems(long long e);
void arena_ccl_set_max_blocks(int b);
hipError_t arena_ccl_broadcast(const ArenaXgmiPeers* P, const float* in, float* out, long long n,
                               int root, hipStream_t stream);
void arena_ccl_set_bcast_direct_max(long long e);
hipError_t arena_ccl_sgd_bf16(const ArenaXgmiPeers* P, float* master, float* mom, long long off,
                              long long n, float lr, const float* lr_ptr, float momentum, float wd,
                              float scale, int nesterov, hipStream_t stream);
void arena_ccl_sgd_shard(long long off, long long n, int world, int r, long long* lo,
                         long long* hi);
hipError_t arena_ccl_sgd_f32(const ArenaXgmiPeers* P, float* mom, long long off, long long n,
                             float lr, const float* lr_ptr, float momentum, float wd, float scale,
                             int nesterov, hipStream_t stream);
void arena_ccl_sgd_f32_shard(long long off, long long n, int world, int r, long long* lo,
                             long long* hi);
hipError_t arena_ccl_allgather(const ArenaXgmiPeers* P, const float* in, float* out, long long m,
                               hipStream_t stream);
void arena_ccl_shard(long long n, int world, int r, long long* lo, long long* hi);
}  // extern "C"
