/* mednet_hip.h -- C ABI of libmednet_hip.so: the MI355X (gfx950) 3D U-Net training hot path.
 *
 * The reference (tobiashepp/torch-mednet) has no FFI of its own: its hot path is torch.nn modules calling
 * ATen.  Each entry point below therefore names the reference call site whose ATen op it replaces
 * (paths relative to the reference root).  The Python host (mednet_hip/_lib.py, ctypes) is the only caller.
 *
 * Conventions
 *   - every pointer is a DEVICE pointer owned by the caller (PyTorch caching allocator); nothing is allocated,
 *     freed or synchronised inside; launches go on `stream` (a hipStream_t passed as void*).
 *   - activations are NDHWC ("channels_last_3d") unless a layout argument says otherwise; dtype arguments name the STORAGE
 *     type of a tensor: MEDNET_F32, MEDNET_BF16 or MEDNET_F16 for activations and their gradients (arithmetic is fp32
 *     accumulation in every mode), MEDNET_U8 / MEDNET_I64 for labels and MEDNET_U8 / MEDNET_F16 for resident volumes where
 *     an entry point says so; parameters and their gradients are always fp32 in PyTorch layout.
 *   - no global state: everything a launch depends on is an argument.  The one exception is mednet_set_option, a table of
 *     integer A/B knobs for measurements; it never carries pointers, results never depend on it, and the product path
 *     (the mednet_hip Python package) sets none.
 *   - return value: MEDNET_OK or a negative MEDNET_E_*; mednet_last_error() gives the text.  The Python shim
 *     raises RuntimeError, matching the reference's assert/exception convention (components.py:30-31,56,65;
 *     loss.py:28,66).
 *   - workspace: *_ws_bytes() gives the scratch size a call needs; the caller passes a buffer at least that big.
 *     Workspaces hold deterministic per-workgroup partials (no float atomics anywhere => bitwise reproducible).
 */
#ifndef MEDNET_HIP_H
#define MEDNET_HIP_H
#include <stddef.h>
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

typedef void* mednet_stream; /* hipStream_t */

enum { MEDNET_F32 = 0, MEDNET_BF16 = 1,
       MEDNET_F16 = 2, /* third activation storage type (fp16, with loss scaling: train.LossScaler); resident image volumes */
       MEDNET_U8 = 3,  /* label / heat-map volumes (mednet_crop_patches), labels of the fused head + Dice kernels */
       MEDNET_I64 = 4, /* labels as the reference's callers pass them (`.long()`, segmentation.py:60) */
       MEDNET_I16 = 5  /* CT volumes as stored: a source type of the intensity entries only */ };
enum { MEDNET_NDHWC = 0, MEDNET_NCDHW = 1 };
enum { MEDNET_ACT_NONE = 0, MEDNET_ACT_RELU = 1, MEDNET_ACT_LEAKY = 2, MEDNET_ACT_ELU = 3 };
enum { MEDNET_POOL_MAX = 0, MEDNET_POOL_AVG = 1 };
/* ALGO_EXACT = ALGO_AUTO, except that fp32-storage contractions use exact fp32 products (v_mfma_f32_32x32x2_f32) instead of
 * the split-bf16 contraction (three bf16 MFMAs per product, ~2^-16 relative): asked for by networks with ReLU / LeakyReLU,
 * whose gradients are discontinuous in the pre-activations (mednet_hip/config.py exact_products). */
enum { MEDNET_ALGO_AUTO = 0, MEDNET_ALGO_DIRECT = 1, MEDNET_ALGO_MFMA = 2, MEDNET_ALGO_EXACT = 3,
       /* the same request OR-ed onto a base choice: MEDNET_ALGO_MFMA | MEDNET_ALGO_EXACT_BIT = matrix-core path required AND
        * exact fp32 products (ALGO_MFMA alone takes the split-bf16 contraction in the fp32 storage mode) */
       MEDNET_ALGO_EXACT_BIT = 4,
       /* (ABI 3, round 6) SPLIT WEIGHTS, OR-ed onto any base choice; 16-bit storage modes only (ignored for fp32 storage).  The
        * matrix cores read 16-bit weight images: in fp16 storage that 11-bit rounding of the WEIGHTS -- not the 16-bit storage of
        * activations and gradients -- is what keeps the gradients of the reference's fp32 step outside 1e-3 (tools/attrib16.py,
        * profiles/r06_ab.md section 2).  With this bit every 3x3x3 forward / data-gradient convolution, ConvTranspose3d forward /
        * data gradient and the first layer also multiply the LOW image elt(w - elt(w)) of the layer's weights (two MFMAs per
        * product; the weight gradients have no weight operand and are unchanged).  The pack must hold the low images: pack with
        * elt_dtype | MEDNET_PACK_LOW (every bf16 pack holds them anyway). */
       MEDNET_ALGO_SPLITW_BIT = 8 };
/* flag of the elt_dtype argument of mednet_conv3d_pack_elt / mednet_conv3d_pack_many: an fp16 pack with the low images as well */
enum { MEDNET_PACK_LOW = 0x100,
       /* (round 6) mednet_conv3d_pack_many only: rewrite ONLY what the 16-bit matrix-core kernels of the training step read -- the
        * high 16-bit images (and the low ones iff MEDNET_PACK_LOW is set) -- and leave the fp32 images of the direct / fp32-matrix
        * kernels and the unrequested low images as they are, i.e. STALE after an optimizer step (2.8 GB per step for a 141 M
        * parameter network against 1.1 GB).  The caller then owns the bookkeeping: before a call that takes another path with such a
        * pack (fp32 tensors, MEDNET_ALGO_DIRECT / exact products, a sample of 4 GB and more, a ConvTranspose3d whose channels are not
        * multiples of 32) it must re-pack that layer in full (mednet_conv3d_pack_elt).  mednet_hip.nn does (`_packed(x)`). */
       MEDNET_PACK_HIGH_ONLY = 0x200 };
enum { MEDNET_REG_L2 = 0, MEDNET_REG_L1 = 1 };
enum { MEDNET_CLASS_DICE = 0, MEDNET_CLASS_CE = 1, MEDNET_CLASS_DICE_CE = 2 };  /* class-loss kind of mednet_head_landmark_cls_* / mednet_head_seg_* */
enum {
  MEDNET_OK = 0, MEDNET_E_SHAPE = -1, MEDNET_E_DTYPE = -2, MEDNET_E_WORKSPACE = -3, MEDNET_E_HIP = -4,
  MEDNET_E_UNSUPPORTED = -5
};
#define MEDNET_NO_IGNORE INT32_MIN

int mednet_abi_version(void);
const char* mednet_last_error(void);
/* 1 if a gfx950 device is visible to this process, 0 otherwise (never throws). */
int mednet_device_ok(void);
/* Kernel-variant knobs for in-process A/B measurements (e.g. "conv32" 0|1); integers only, results never depend on them,
 * and the table is read without a lock: set them from one thread while no launch is being planned (tools/, tests/). */
int mednet_set_option(const char* name, int value);
/* the value a launcher would read now (default_value when the option was never set); tests and tools */
int mednet_get_option(const char* name, int default_value);

/* ---- nn.Conv3d(k=3,p=1 | k=1,p=0, stride 1)  components.py:8-9,44 ; model.py:77,179 ------------------------ */
/* Weight packing: PyTorch (Cout,Cin,k,k,k) [or ConvTranspose3d's (Cin,Cout,k,k,k) when transposed_src=1] ->
 * opaque buffer holding the tap-major layouts the forward, data-gradient and MFMA kernels read. */
size_t mednet_conv3d_pack_bytes(int cin, int cout, int ksize);  /* the buffer must be 16-byte aligned (hipMalloc / torch allocations are) */
/* mednet_conv3d_pack writes the matrix-core fragment images in bf16; _elt takes the storage type of the activations the
 * layer will see.  MEDNET_BF16 and MEDNET_F32 write the same thing: bf16 images of the HIGH halves bf16(w) plus images of
 * the LOW halves bf16(w - bf16(w)); 16-bit calls read the high images, fp32-storage calls (the mode that meets the reference
 * within 1e-3) contract against both (split-bf16 product, conv_x3_mfma.hip) -- so a buffer packed either way serves both
 * storage modes.  MEDNET_F16 (BASELINE config 5 stores fp16) writes fp16 high images and serves fp16-storage calls ONLY: the
 * exact-product fp32 kernels (MEDNET_ALGO_EXACT) still work on it, they read the fp32 tap-major images every pack holds, but
 * an automatic-algorithm fp32-storage call on an fp16 pack is a caller error.  The buffer size is the same in every case. */
int mednet_conv3d_pack_elt(const float* w, void* packed, int cin, int cout, int ksize, int transposed_src, int elt_dtype,
                           mednet_stream stream);
int mednet_conv3d_pack(const float* w, void* packed, int cin, int cout, int ksize, int transposed_src,
                       mednet_stream stream);
/* Every 3x3x3 layer with matrix-core images in ONE launch (after an optimizer step all weights have moved; the reference
 * has no counterpart: torch.nn keeps no packed copies).  mednet_conv3d_pack_table turns the caller's job list into the
 * table the kernel reads (table_host: mednet_conv3d_pack_table_bytes(njobs) bytes of host memory, to be copied to the
 * device once; *blocks = the block count of the launch, to be handed back to mednet_conv3d_pack_many);
 * mednet_conv3d_pack_many repeats what mednet_conv3d_pack_elt does for each job. */
typedef struct mednet_pack_job {
  const float* w;      /* parameter, PyTorch layout, device */
  void* packed;        /* its pack buffer (mednet_conv3d_pack_bytes), device */
  int cin, cout, ksize, transposed_src;
} mednet_pack_job;
size_t mednet_conv3d_pack_table_bytes(int njobs);
int mednet_conv3d_pack_table(const mednet_pack_job* jobs, int njobs, void* table_host, unsigned* blocks);
int mednet_conv3d_pack_many(const void* table_device, int njobs, unsigned blocks, int elt_dtype, mednet_stream stream);
/* y[n,z,y,x,co] = bias[co] + sum_{tap,ci} x[n,z+dz-1,y+dy-1,x+dx-1,ci] * W[co,ci,tap].
 * dgrad=1 runs the data gradient with the same kernel: pass x := dy, cin := Cout, cout := Cin of the layer. */
/* gn_partial (nullable): when the call takes the MFMA path the epilogue also writes the GroupNorm partial sums of the
 * output, [n][chunks][cout][2] = {sum y, sum y^2} per brick, chunks = mednet_conv3d_fused_stats_chunks(...) (0 = this
 * call cannot fuse them); mednet_gn_finalize turns them into statistics without another pass over y.  The sums are
 * kept per channel PAIR (entry 2j = channels 2j and 2j+1 together, entry 2j+1 = 0): exact for GroupNorm whenever the
 * channels per group are even -- ask for them only then. */
/* Audit aid (no device needed): the launch plan of the 16-bit matrix-core kernel that produces a 3x3x3 layer's partial rows,
 * from the launcher's own planning code.  gnb: the data-gradient form with GroupNorm-backward sums (pass the kernel's Cin /
 * Cout, i.e. the layer's Cout / Cin); stride 2: the ConvTranspose3d data gradient with GroupNorm-3 sums (d, h, w = the
 * low-resolution grid).  out13 = {kind (2: one row per wave and brick, row = 4 * brick-in-sample + wave; 3: accumulate mode,
 * a wave keeps its sums over its workgroup's items and writes row ((wg >> 3) / ncb * 8 + (wg & 7)) * 4 + wave for EVERY
 * sample; 4: the 32 -> 32 specialisation, row = 4 * wg + wave for every sample; 5 / 6: the two-block kernel with the rows of
 * 2 / 3 and "channel blocks" counting PAIRS of 32-channel blocks; 7: the ConvTranspose3d 64 -> 32 data gradient, row = 2 * wg +
 * z-plane of its bricks for every sample, both channel blocks), grid, work items, channel blocks, bricks,
 * bricks per sample, accumulate flag, rows per sample, and for kind 4 bricks per XCD, z-slab height, brick counts in x, y, z}.
 * Work item i of the general kernel = (brick (i >> 3) / ncb * 8 + (i & 7), channel block (i >> 3) % ncb); workgroup b takes
 * items b, b + grid, ... and stops at the first brick >= bricks (padding items). */
int mednet_conv3d_stats_plan(int n, int d, int h, int w, int cin, int cout, int dtype, int gnb, int stride, int* out13);
int mednet_conv3d_fused_stats_chunks(int n, int d, int h, int w, int cin, int cout, int ksize, int x_dtype,
                                     int y_dtype, int algo);
int mednet_conv3d_fwd(const void* x, const void* packed, const float* bias, void* y, int n, int d, int h, int w,
                      int cin, int cout, int ksize, int x_dtype, int x_layout, int y_dtype, int y_layout,
                      int dgrad, int algo, float* gn_partial, mednet_stream stream);
/* Multi-channel network input (Cin = 2, 3, 4: PET/CT, multi-sequence MRI) in the 16-bit storage modes: 1 exactly for the calls
 * that mednet_conv3d_fwd gives to the matrix-core first-layer kernel -- 3x3x3, no bias, fp32 x, 16-bit channels-last y,
 * Cout % 16 == 0, algo AUTO or MFMA (with or without MEDNET_ALGO_SPLITW_BIT), tuning option conv_cm = 1 (the default; 0 restores
 * the dispatch without this kernel).  For such a call x may be passed in EITHER layout -- planar N x C x D x H x W as a batch
 * holds it (x_layout = MEDNET_NCDHW, no layout copy) or channels-last --, with identical results; gn_partial is accepted and
 * mednet_conv3d_fused_stats_chunks gives its row count.  mednet_conv3d_wgrad takes the same two layouts for this layer when
 * Cout <= 64 (matrix-core kernel, obeys option wgrad_c1_mfma). */
int mednet_conv3d_cm_supported(int cin, int cout, int ksize, int x_dtype, int y_dtype, int algo);
/* conv 3x3x3 without bias + activation (MEDNET_ACT_*) in the epilogue, bf16 NDHWC in and out, matrix-core path only:
 * the conv -> ReLU / LeakyReLU / ELU step of the 'gcr'-style orders (components.py:12-67; UNet3D's default).  gn_partial as
 * in mednet_conv3d_fwd; the statistics are those of the ACTIVATED output (the next GroupNorm's input).  Ask
 * mednet_conv3d_act_supported first; unsupported shapes return MEDNET_E_UNSUPPORTED (use conv3d_fwd + act_fwd). */
int mednet_conv3d_act_supported(int n, int d, int h, int w, int cin, int cout, int algo);
int mednet_conv3d_act_fwd(const void* x, const void* packed, void* y, int n, int d, int h, int w, int cin, int cout,
                          int act, int algo, float* gn_partial, int dtype, mednet_stream stream);
/* dx = dgrad(dy) + add: the data gradient of a 3x3x3 conv (layer Cin -> Cout; dy has Cout channels, dx and add have Cin)
 * with a second gradient of the same tensor summed in the epilogue (fp32 add, one bf16 rounding): in ExtResNetBlock the
 * first conv's output feeds conv2 AND the residual add (components.py:170-178), so its two gradients meet here instead
 * of in two more tensor reads of the GroupNorm backward.  bf16 NDHWC, matrix-core path only
 * (mednet_conv3d_act_supported(n,d,h,w,Cout,Cin,algo) tells). */
int mednet_conv3d_dgrad_add(const void* dy, const void* packed, const void* add, void* dx, int n, int d, int h, int w,
                            int cin, int cout, int algo, int dtype, mednet_stream stream);
/* mednet_conv3d_dgrad_add (add nullable) that ALSO takes the first pass of the backward of the GroupNorm (+ activation)
 * in front of the layer (components.py:57,36-40: `SingleConv` k-1 of the block produced this conv's input): with gn_y the
 * conv output that GroupNorm normalised (shape of dx), gn_coef[n][Cin] = {ca, cb} its forward affine (mednet_gn_stats /
 * _finalize) and gn_act its activation, the epilogue forms du = dx * act'(ca * gn_y + cb) from the stored dx rows and writes
 * gn_partial[n][rows][Cin][2] = per-channel {sum du, sum du * gn_y} (rows = mednet_conv3d_dgrad_gn_rows(...), 0 = not
 * supported for this shape).  mednet_gn_act_bwd_fused consumes it: no stand-alone pass re-reads dx and gn_y. */
int mednet_conv3d_dgrad_gn_rows(int n, int d, int h, int w, int cin, int cout, int algo);
/* ... by storage type: MEDNET_F32 = the fp32 storage mode, where the split-bf16 data-gradient kernel takes the sums (and the
 * summed second gradient) the same way; 16-bit types answer as mednet_conv3d_dgrad_gn_rows.  mednet_conv3d_dgrad_add_supported:
 * 1 if mednet_conv3d_dgrad_add takes this layer in this storage type. */
int mednet_conv3d_dgrad_gn_rows_dt(int n, int d, int h, int w, int cin, int cout, int algo, int dtype);
int mednet_conv3d_dgrad_add_supported(int n, int d, int h, int w, int cin, int cout, int algo, int dtype);
int mednet_conv3d_dgrad_gn(const void* dy, const void* packed, const void* add, void* dx, const void* gn_y,
                           const float* gn_coef, int gn_act, float* gn_partial, int n, int d, int h, int w, int cin,
                           int cout, int algo, int dtype, mednet_stream stream);
/* GroupNorm-3 of an ExtResNetBlock (out = act(GroupNorm(conv3(z2)) + z1), components.py:170-178): its backward's first
 * pass -- du = dout * act'(out), per-channel {sum du, sum du * y3} -- taken by the kernel that PRODUCES dout, from the
 * stored (rounded) dout rows: the data gradient of the 1x1x1 head (model.py:204-207; dy = planar fp32 logit gradients,
 * dx / gn_y = y3 / gn_z = out channels-last 16-bit, cin = block channels, cout = classes) for the last decoder block, and
 * the pooling backward + skip-gradient join (mednet_pool2_bwd; model.py:194-205; x = the block output) for the encoder
 * blocks that feed a pooling.  gn_partial[n][rows][C][2] with rows from the *_rows call (0 = not supported for this shape / dtype; even
 * d, h, w for the pooling form); mednet_gn_act_bwd_fused_res consumes it and also writes the residual-branch gradient. */
int mednet_head_dgrad_gn_rows(int n, int d, int h, int w, int cin, int dtype);
int mednet_head_dgrad_gn(const void* dy, const void* packed, void* dx, const void* gn_y, const void* gn_z, int gn_act,
                         float* gn_partial, int n, int d, int h, int w, int cin, int cout, int dtype, mednet_stream stream);
/* ... and the ConvTranspose3d data gradient (mednet_convt3d_dgrad: model.py:202-207, the decoder's upsampling consumes the
 * output of the block below; (n,d,h,w) = dx dims, gn_y / gn_z = that block's y3 / output, Cin channels), matrix-core path. */
int mednet_convt3d_dgrad_gn_rows(int n, int d, int h, int w, int cin, int cout, int dtype, int algo);
int mednet_convt3d_dgrad_gn(const void* dy, const void* packed, void* dx, const void* gn_y, const void* gn_z, int gn_act,
                            float* gn_partial, int n, int d, int h, int w, int cin, int cout, int dtype, int algo,
                            mednet_stream stream);
int mednet_pool2_bwd_gn_rows(int n, int d, int h, int w, int c, int dtype);
int mednet_pool2_bwd_gn(const void* dy, const void* x, const void* add, void* dx, const void* gn_y, int gn_act,
                        float* gn_partial, int n, int d, int h, int w, int c, int mode, int dtype, mednet_stream stream);
/* dw[co,ci,tap] = sum_{n,v} dy[n,v,co] * x[n,v+tap,ci]; dbias[co] = sum dy (nullable).
 * `workgroups` (>= 0) is part of the launch plan and therefore an ARGUMENT of the call and of its workspace query (the same
 * value to both): 0 = the library's plan, one persistent workgroup per CU; N > 0 = about N workgroups -- the trainer passes
 * half the CUs for launches that run on a second stream beside the main one (a weight-gradient workgroup takes a CU's whole
 * register file; mednet_hip/ops.py _OnSide).  Results are deterministic for a fixed value (fixed-order reduce of the
 * per-workgroup partial slabs); another value changes the rounding of the sums, once.  Kernels that do not split their work
 * this way (first layer, 1x1x1 head, direct kernels) ignore it. */
size_t mednet_conv3d_wgrad_ws_bytes(int n, int d, int h, int w, int cin, int cout, int ksize, int workgroups);
/* 1 if this weight gradient runs on the co-resident kernel (wgrad_mfma4_kernel: 4 waves of < 256 registers, 104 KB of LDS --
 * bandwidth-bound kernels of another stream run on the same CUs beside it); 0 if it takes its CUs whole.  A caller that runs
 * weight gradients on a second stream passes workgroups = 0 (all CUs) in the first case and about half the CUs in the second. */
int mednet_conv3d_wgrad_coresident(int n, int d, int h, int w, int cin, int cout, int ksize, int x_dtype, int dy_dtype, int algo);
/* Launch plan of the 3x3x3 weight gradient (16-bit matrix-core path) made by the launcher's own planning code, for audits without
 * a device (tests/test_plan_audit.py): out10 = {kind (4: wgrad_mfma4_kernel, z-columns; 2: wgrad_mfma2_kernel, bricks), workgroups,
 * channel-block pairs, workgroups per pair, work items per pair, tiles_x, tiles_y, z-slabs (kind 4) or tiles_z (kind 2), planes
 * per slab (kind 4) or brick width (kind 2), XCD remap of the item order (kind 4)}. */
int mednet_conv3d_wgrad_plan(int n, int d, int h, int w, int cin, int cout, int dtype, int workgroups, int* out10);
/* The Cin = 1, 3x3x3 weight gradient with GroupNorm's backward apply folded into its staging: dz / y = gradient of, and input
 * to, act(GroupNorm(y)) (16-bit NDHWC, Cout channels), coef = the forward affine {ca, cb}, bcoef from
 * mednet_gn_bwd_coefficients.  dw gets what mednet_conv3d_wgrad(x, dy) returns for the dy mednet_gn_act_bwd_fused stores --
 * bit for bit -- without dy ever reaching memory.  Workspace: mednet_conv3d_wgrad_ws_bytes(n, d, h, w, 1, cout, 3, 0).
 * _supported: Cout in {16, 32, 64}, 16-bit dtype, x fp32 or that dtype. */
int mednet_conv3d_wgrad_c1_gn_supported(int cout, int x_dtype, int dtype);
int mednet_conv3d_wgrad_c1_gn(const void* x, const void* dz, const void* y, const float* coef, const float* bcoef, float* dw,
                              int n, int d, int h, int w, int cout, int act, int x_dtype, int dtype, void* ws, size_t ws_bytes,
                              mednet_stream stream);
/* The same for the multi-channel first layer (Cin = 2, 3, 4): x is fp32 in `x_layout` (planar or channels-last), dw is
 * (cout, cin, 3, 3, 3); dz and y are read from memory once, all Cin channels of x are contracted against the one staged brick.
 * Workspace: mednet_conv3d_wgrad_ws_bytes(n, d, h, w, cin, cout, 3, 0).  _supported: Cin in {2, 3, 4}, Cout in {16, 32, 48, 64},
 * fp32 x, 16-bit dtype, options conv_cm and wgrad_c1_mfma on.
 * mednet_conv3d_wgrad_cm_plan: the launcher's own plan of this weight gradient (no device needed), out4 = {workgroups,
 * 32-channel blocks per workgroup, workgroups per CU the kernel is compiled for, dynamic LDS bytes}; gn = 1: the GroupNorm form,
 * gn = 0: the plain form mednet_conv3d_wgrad runs. */
int mednet_conv3d_wgrad_cm_gn_supported(int cin, int cout, int x_dtype, int dtype);
int mednet_conv3d_wgrad_cm_plan(int n, int d, int h, int w, int cin, int cout, int dtype, int gn, int* out4);
int mednet_conv3d_wgrad_cm_gn(const void* x, int x_layout, const void* dz, const void* y, const float* coef, const float* bcoef,
                              float* dw, int n, int d, int h, int w, int cin, int cout, int act, int x_dtype, int dtype, void* ws,
                              size_t ws_bytes, mednet_stream stream);
int mednet_conv3d_wgrad(const void* x, const void* dy, float* dw, float* dbias, int n, int d, int h, int w,
                        int cin, int cout, int ksize, int x_dtype, int x_layout, int dy_dtype, int dy_layout,
                        int algo, int workgroups, void* ws, size_t ws_bytes, mednet_stream stream);

/* ---- nn.ConvTranspose3d(k=3,s=2,p=1,output_padding=1,bias) + `x += encoder_features`  components.py:259-264,283-284 */
/* (n,d,h,w) are the INPUT dims; output is (2d,2h,2w).  `skip` (nullable, y's dtype/shape) is added in the epilogue. */
int mednet_convt3d_fwd(const void* x, const void* packed, const float* bias, const void* skip, void* y, int n,
                       int d, int h, int w, int cin, int cout, int x_dtype, int y_dtype, int algo,
                       mednet_stream stream);
int mednet_convt3d_dgrad(const void* dy, const void* packed, void* dx, int n, int d, int h, int w, int cin,
                         int cout, int dy_dtype, int dx_dtype, int algo, mednet_stream stream);
/* (`workgroups`: as for mednet_conv3d_wgrad) */
size_t mednet_convt3d_wgrad_ws_bytes(int n, int d, int h, int w, int cin, int cout, int workgroups);
int mednet_convt3d_wgrad(const void* x, const void* dy, float* dw, float* dbias, int n, int d, int h, int w,
                         int cin, int cout, int x_dtype, int dy_dtype, int algo, int workgroups, void* ws,
                         size_t ws_bytes, mednet_stream stream);

/* ---- nn.GroupNorm(G,C,eps) fused with the following activation and the residual add
 *      components.py:57 (GroupNorm), :36-40 (ReLU/LeakyReLU(0.1)/ELU), :177-178 (out += residual; non_linearity) */
size_t mednet_gn_ws_bytes(int n, int c, size_t spatial);
/* stats[n][g] = {mean, rstd}; coef[n][c] = {gamma*rstd, beta - mean*gamma*rstd} (both outputs, fp32).  The sums are taken of
 * x - p, p one element of the group itself (mednet_bn_stats: of the channel): the variance does not degrade with mean / std. */
int mednet_gn_stats(const void* x, const float* gamma, const float* beta, float* stats, float* coef, int n,
                    size_t spatial, int c, int groups, float eps, int dtype, void* ws, size_t ws_bytes,
                    mednet_stream stream);
/* the second half of mednet_gn_stats for partial sums produced elsewhere (fused conv epilogue):
 * partial is [n][chunks][c][2] = {sum x, sum x^2}; ws needs n*c*2 floats.  var = sum x^2 / N - mean^2: its error grows as
 * (mean / std)^2 -- for data far from zero use mednet_gn_stats on the tensor. */
int mednet_gn_finalize(const float* partial, int chunks, const float* gamma, const float* beta, float* stats,
                       float* coef, int n, size_t spatial, int c, int groups, float eps, void* ws, size_t ws_bytes,
                       mednet_stream stream);
/* z = act(coef0*x + coef1 [+ residual]) */
int mednet_gn_act_fwd(const void* x, const float* coef, const void* residual, void* z, int n, size_t spatial,
                      int c, int act, int x_dtype, int z_dtype, mednet_stream stream);
/* du = (dz [+ dz2]) * act';  dgamma/dbeta;  dx = GroupNorm backward of du;  dres (nullable) := du.
 * act' comes from the activated output z when given (ATen's in-place semantics), else -- no residual branch -- it is
 * recomputed from x and the forward coefficients `coef`, which saves reading z back (one tensor less per pass). */
/* in_act (both forms below): MEDNET_ACT_* of the activation whose OUTPUT is x (conv -> ReLU -> this GroupNorm in the 'gcr'
 * orders, components.py:36-40): dx is multiplied by its derivative here, sparing the conv layer's backward a pass. */
int mednet_gn_act_bwd(const void* dz, const void* dz2, const void* x, const void* z, const float* coef,
                      const float* stats, const float* gamma, void* dx, void* dres, float* dgamma, float* dbeta, int n,
                      size_t spatial, int c, int groups, int act, int in_act, int dtype, void* ws, size_t ws_bytes,
                      mednet_stream stream);
/* mednet_gn_act_bwd without its first pass: `partial` [n][rows][c][2] = per-channel {sum du, sum du * x} comes from the
 * kernel that produced dz (mednet_conv3d_dgrad_gn); act' is recomputed from x and `coef` (z is not read). */
int mednet_gn_act_bwd_fused(const void* dz, const void* x, const float* coef, const float* stats, const float* gamma,
                            const float* partial, int rows, void* dx, float* dgamma, float* dbeta, int n,
                            size_t spatial, int c, int groups, int act, int in_act, int dtype, void* ws, size_t ws_bytes,
                            mednet_stream stream);
/* Passes 1b + 2 of mednet_gn_act_bwd_fused alone: bcoef[n][c][3] = {k1, k2, k3} with dx = k1 * du + k2 * x + k3
 * (du = dz * act'(coef_a * x + coef_b)), and dgamma / dbeta.  For a consumer that applies the coefficients while it reads
 * (dz, x) for its own purpose -- mednet_conv3d_wgrad_c1_gn below -- so the apply pass and its dx tensor disappear.  The first
 * SingleConv of the network (components.py:57 after model.py:63's first encoder) needs no gradient of the network input:
 * its GroupNorm backward only feeds the weight gradient. */
int mednet_gn_bwd_coefficients(const float* stats, const float* gamma, const float* partial, int rows, float* bcoef,
                               float* dgamma, float* dbeta, int n, size_t spatial, int c, int groups, void* ws,
                               size_t ws_bytes, mednet_stream stream);
int mednet_gn_act_bwd_fused_res(const void* dz, const void* x, const void* z, const float* coef, const float* stats,
                                const float* gamma, const float* fused_partial, int rows, void* dx, void* dres,
                                float* dgamma, float* dbeta, int n, size_t spatial, int c, int groups, int act, int dtype,
                                void* ws, size_t ws_bytes, mednet_stream stream);
/* ... when dz is the pooling backward + skip join of an encoder level and was NOT materialised: mednet_pool2_bwd_gn called with
 * dx = NULL takes the sums only, and this apply pass rebuilds dz per 2x2x2 window from the pooled gradient dy_pool, the arg-max of
 * the block output z (read for act' anyway) and the skip gradient (nullable), rounded as the pooling backward would have stored
 * it.  dx (= dy3) and dres are bit-identical to mednet_pool2_bwd_gn + mednet_gn_act_bwd_fused_res.  Even d, h, w; C % 8 == 0. */
int mednet_gn_act_bwd_fused_res_pool(const void* dy_pool, const void* skip_grad, const void* x, const void* z, const float* stats,
                                     const float* gamma, const float* fused_partial, int rows, void* dx, void* dres, float* dgamma,
                                     float* dbeta, int n, int d, int h, int w, int c, int groups, int act, int pool_mode, int dtype,
                                     void* ws, size_t ws_bytes, mednet_stream stream);
/* ... when dz is the feature gradient of the small fused head (mednet_head_dice_* / mednet_head_ce_* / mednet_head_dice_ce_*) and was
 * NOT materialised: mednet_head_*_bwd_sums took the sums only, and this apply pass rebuilds each row of dz from the voxel's logits
 * (planar fp32, cout planes), its label and the head's 4 x 32 weights (`packed`), with the loss operands of the head's backward
 * (weight, saved, dloss, eps, sigmoid, ignore_index; class_kind = MEDNET_CLASS_*) -- the same device code as the head's backward,
 * rounded as it would have stored the row.  dx (= dy3), dres, dgamma and dbeta are bit-identical to mednet_head_*_bwd +
 * mednet_gn_act_bwd_fused_res.  Additive to ABI 3.  _supported: c == 32, 1 <= cout <= 4, bf16 / f16 storage, uint8 / int64 labels. */
int mednet_gn_act_bwd_fused_res_head_supported(int c, int cout, int dtype, int label_dtype);
int mednet_gn_act_bwd_fused_res_head(const float* logits, const void* labels, int label_dtype, int64_t label_stride_n,
                                     const void* packed, const float* weight, const float* saved, const float* dloss, float eps,
                                     int sigmoid, int ignore_index, int class_kind, int cout, const void* x, const void* z,
                                     const float* stats, const float* gamma, const float* fused_partial, int rows, void* dx, void* dres,
                                     float* dgamma, float* dbeta, int n, size_t spatial, int c, int groups, int act, int dtype, void* ws,
                                     size_t ws_bytes, mednet_stream stream);
/* ---- nn.BatchNorm3d(C, eps, momentum) fused with the following activation and the residual add
 *      components.py:58-63 (order char 'b').  Channels-last storage: the batch is one [N * S][C] array.  stats[n][c] =
 *      {mean, rstd} and coef[n][c] = {gamma*rstd, beta - mean*gamma*rstd} are written REPLICATED per sample (all n rows equal), so
 *      mednet_gn_act_fwd, mednet_gn_act_pool_fwd and the data-gradient forms that take a GroupNorm's coef (mednet_conv3d_dgrad_gn
 *      and relatives) apply / consume them unchanged.  Workspace of every call: mednet_gn_ws_bytes(n, c, spatial). */
/* Training mode: batch statistics over all N * S voxels (biased variance) and, when running_mean / running_var are given (both
 * or neither, fp32 [c]), running = (1 - momentum) * running + momentum * {mean, unbiased variance}; num_batches_tracked (nullable,
 * one int64) += 1.  Everything happens on the device in stream order (the call can be captured in a graph). */
int mednet_bn_stats(const void* x, const float* gamma, const float* beta, float* running_mean, float* running_var,
                    long long* num_batches_tracked, float momentum, float* stats, float* coef, int n, size_t spatial, int c,
                    float eps, int dtype, void* ws, size_t ws_bytes, mednet_stream stream);
/* Evaluation mode: the same stats / coef rows from the running statistics; apply with mednet_gn_act_fwd. */
int mednet_bn_eval_coef(const float* running_mean, const float* running_var, const float* gamma, const float* beta, float* stats,
                        float* coef, int n, int c, float eps, mednet_stream stream);
/* du = dz * act' (from z when given, else recomputed from x and coef);  dbeta = sum du, dgamma = sum du * xhat over all samples;
 * dx = k1 * du + k2 * x + k3 (BatchNorm backward; frozen != 0: the statistics were constants -- evaluation mode --, dx = k1 * du);
 * dres (nullable) := du.  in_act as for mednet_gn_act_bwd.  Sums in a fixed order: two runs give the same bits. */
int mednet_bn_act_bwd(const void* dz, const void* x, const void* z, const float* coef, const float* stats, const float* gamma,
                      void* dx, void* dres, float* dgamma, float* dbeta, int n, size_t spatial, int c, int act, int in_act,
                      int frozen, int dtype, void* ws, size_t ws_bytes, mednet_stream stream);
/* ... without its first pass: `partial` [n][rows][c][2] = per-channel {sum du, sum du * x} from the kernel that produced dz
 * (mednet_conv3d_dgrad_gn and relatives), summed here over rows AND samples. */
int mednet_bn_act_bwd_fused(const void* dz, const void* x, const float* coef, const float* stats, const float* gamma,
                            const float* partial, int rows, void* dx, float* dgamma, float* dbeta, int n, size_t spatial, int c,
                            int act, int in_act, int frozen, int dtype, void* ws, size_t ws_bytes, mednet_stream stream);

/* stand-alone activation (orders such as 'cr', 'crg'); in-place allowed (x == z). */
int mednet_act_fwd(const void* x, void* z, size_t count, int act, int dtype, mednet_stream stream);
int mednet_act_bwd(const void* dz, const void* z, void* dx, size_t count, int act, int dtype,
                   mednet_stream stream);
/* out = a + b (gradient joins the graph needs: residual + skip fan-in). */
int mednet_add(const void* a, const void* b, void* out, size_t count, int dtype, mednet_stream stream);

/* ---- nn.MaxPool3d(2) / nn.AvgPool3d(2)  components.py:208-212 ----------------------------------------------- */
int mednet_pool2_fwd(const void* x, void* y, int n, int d, int h, int w, int c, int mode, int dtype,
                     mednet_stream stream);
/* dx has the INPUT shape; ties route to the first maximum in (z,y,x) scan order like ATen.  `add` (nullable, input
 * shape): a second gradient of the same tensor -- the decoder's skip join of model.py:199-205 -- summed in the same pass. */
/* GroupNorm apply (+ residual + activation, as mednet_gn_act_fwd) fused with the 2x2x2 pooling that consumes its output (an
 * encoder block's last layer followed by the next level's pooling, components.py:177-178 -> :222-224): writes z AND the pooled
 * tensor in one pass; both bit-identical to mednet_gn_act_fwd + mednet_pool2_fwd.  Even d, h, w; C a multiple of 8. */
int mednet_gn_act_pool_supported(int d, int h, int w, int c, int dtype);
int mednet_gn_act_pool_fwd(const void* x, const float* coef, const void* residual, void* z, void* pooled, int n, int d, int h,
                           int w, int c, int act, int mode, int dtype, mednet_stream stream);
int mednet_pool2_bwd(const void* dy, const void* x, const void* add, void* dx, int n, int d, int h, int w, int c,
                     int mode, int dtype, mednet_stream stream);
/* ... with the derivative of the activation whose OUTPUT x is (a fused conv -> activation layer, components.py:57-63) folded into
 * dx = (pooling backward + add) * act'(x), rounded like the stand-alone join followed by mednet_act_bwd.  Even d, h, w.
 * add_channels (0 or c: dense): `add` points at the first of c channels inside voxel rows of add_channels channels -- the leading
 * slice of the gradient of UNet3D's concatenation (components.py:277-280), read where it lies. */
int mednet_pool2_bwd_act(const void* dy, const void* x, const void* add, int add_channels, void* dx, int n, int d, int h, int w, int c,
                         int mode, int in_act, int dtype, mednet_stream stream);

/* ---- F.interpolate(nearest, size=enc) + torch.cat((enc, x), 1)  components.py:277-280 (UNet3D decoder) ------- */
int mednet_upcat_fwd(const void* enc, const void* x, void* out, int n, int d, int h, int w, int c_enc, int xd,
                     int xh, int xw, int c_x, int dtype, mednet_stream stream);
/* mednet_upcat_fwd that also takes the GroupNorm partial sums of the tensor it writes (UNet3D's decoder opens with a GroupNorm over
 * the concatenation, components.py:46-57 after :277-280): partial[n][mednet_upcat_stats_chunks][c_enc + c_x][2] = {sum, sum of
 * squares}, to be finalised by mednet_gn_finalize.  chunks == 0: not for this shape (channel counts must be multiples of 8). */
int mednet_upcat_stats_chunks(int n, int d, int h, int w, int c_enc, int c_x, int dtype);
int mednet_upcat_fwd_stats(const void* enc, const void* x, void* out, float* partial, int n, int d, int h, int w, int c_enc, int xd,
                           int xh, int xw, int c_x, int dtype, mednet_stream stream);
/* (denc == NULL: only dx; the caller reads the encoder part of dout where it lies) */
int mednet_upcat_bwd(const void* dout, void* denc, void* dx, int n, int d, int h, int w, int c_enc, int xd, int xh,
                     int xw, int c_x, int dtype, mednet_stream stream);

/* ---- losses.  logits are fp32 with element strides (stride_n, stride_c) and unit voxel stride (NCDHW or a
 *      channel slice of it); labels are int64 N x spatial ------------------------------------------------------ */
size_t mednet_loss_ws_bytes(int n, int c, size_t spatial);
/* DiceLoss  loss.py:91-130 (+ :24-48, :58-88): softmax|sigmoid -> one-hot -> per-channel 2*w*I/clamp(D,eps) ->
 * mean(1-dice).  saved[c] = {I_c, D_c} for the backward; dice_out (nullable) gets the per-channel dice. */
int mednet_dice_fwd(const float* logits, const int64_t* labels, const float* weight, float* loss, float* saved,
                    float* dice_out, int n, int c, size_t spatial, int64_t stride_n, int64_t stride_c, float eps,
                    int sigmoid, int ignore_index, void* ws, size_t ws_bytes, mednet_stream stream);
/* dlogits has the layout of the logits view it belongs to (the same stride_n / stride_c; a contiguous N x C x spatial tensor
 * for contiguous logits): a channel slice of the network output gets its gradient written into the matching slice of a
 * full-size buffer (landmarks.py:71-72).  Scaled by *dloss (device scalar). */
int mednet_dice_bwd(const float* logits, const int64_t* labels, const float* weight, const float* saved,
                    const float* dloss, float* dlogits, int n, int c, size_t spatial, int64_t stride_n,
                    int64_t stride_c, float eps, int sigmoid, int ignore_index, mednet_stream stream);
/* The same with the labels as they lie: MEDNET_I64 or MEDNET_U8, element stride label_stride_n between samples (the last channel
 * of a uint8 N x C x D x H x W label volume: `batch['label'][:, -1]`, segmentation.py:60 / landmarks.py:70, without the cast). */
int mednet_dice_fwd_lt(const float* logits, const void* labels, int label_dtype, int64_t label_stride_n, const float* weight,
                       float* loss, float* saved, float* dice_out, int n, int c, size_t spatial, int64_t stride_n,
                       int64_t stride_c, float eps, int sigmoid, int ignore_index, void* ws, size_t ws_bytes, mednet_stream stream);
int mednet_dice_bwd_lt(const float* logits, const void* labels, int label_dtype, int64_t label_stride_n, const float* weight,
                       const float* saved, const float* dloss, float* dlogits, int n, int c, size_t spatial, int64_t stride_n,
                       int64_t stride_c, float eps, int sigmoid, int ignore_index, mednet_stream stream);
/* Dice + cross-entropy, the compound class loss, in one pass over the logits each way (additive to ABI 3):
 *   loss = DiceLoss(weight, eps, softmax)(x, y) + nn.CrossEntropyLoss(weight)(x, y), unit coefficients, one class-weight vector.
 * Softmax only and no ignore_index (the entries have neither argument).  Logits, labels and dlogits as mednet_dice_fwd_lt / _bwd_lt
 * take them; 1 <= c <= 32.  saved: 2 c + 1 floats, [c][2] = {I_c, D_c} followed by sum w_y.  dice_out (nullable): the per-channel
 * dice.  Workspace: mednet_dice_ce_ws_bytes (the Dice rows and the CE rows of every workgroup; mednet_loss_ws_bytes is too small).
 * A label outside [0, c) makes the loss and every logit gradient NaN.
 * Bit-identity: the two terms are accumulated with the instructions and in the order of mednet_dice_fwd_lt (sigmoid 0,
 * MEDNET_NO_IGNORE) and mednet_ce_fwd and combined by the same fp64 fixed-order sums, so *loss is the fp32 sum of those two
 * entries' losses and saved holds their saved values; dlogits is, element by element, the fp32 sum of mednet_dice_bwd_lt's and
 * mednet_ce_bwd's results for the same *dloss (what autograd forms of the two-kernel composition), written with one store. */
size_t mednet_dice_ce_ws_bytes(int n, int c, size_t spatial);
int mednet_dice_ce_fwd_lt(const float* logits, const void* labels, int label_dtype, int64_t label_stride_n, const float* weight,
                          float* loss, float* saved, float* dice_out, int n, int c, size_t spatial, int64_t stride_n,
                          int64_t stride_c, float eps, void* ws, size_t ws_bytes, mednet_stream stream);
int mednet_dice_ce_bwd_lt(const float* logits, const void* labels, int label_dtype, int64_t label_stride_n, const float* weight,
                          const float* saved, const float* dloss, float* dlogits, int n, int c, size_t spatial, int64_t stride_n,
                          int64_t stride_c, float eps, mednet_stream stream);
/* The 1x1x1 head (model.py:207 final_conv: nn.Conv3d(f_maps[0], out_channels, 1)) fused with DiceLoss (loss.py:114-130) --
 * what `outputs = self(inputs); loss = self.loss(outputs, labels)` (segmentation.py:61-62) runs between the last decoder block and
 * the scalar loss.  Forward: logits (N x C x spatial fp32, written once, for the caller) + loss + saved[c] = {I_c, D_c} in one pass
 * over the channels-last features z (N x spatial x Cin; f32 / bf16 / f16).  Backward: dz = W^T dlogits (Cin in {16, 32, 64},
 * C <= 4 classes), dW, dbias and -- when gn_y is given -- the first pass of the producing ExtResNetBlock's GroupNorm-3 backward
 * (gn_partial[n][mednet_head_dice_gn_rows][Cin][2], as mednet_head_dgrad_gn) in ONE pass; the logit gradient is never stored.
 * labels: MEDNET_I64 or MEDNET_U8, N x spatial with element stride label_stride_n between samples (the last channel of a
 * uint8 label volume is consumed where it lies).  packed: the head's pack buffer (mednet_conv3d_pack, ksize 1).
 * Logits, loss, dz and the GroupNorm sums are bit-identical to mednet_conv3d_fwd + mednet_dice_fwd / mednet_dice_bwd +
 * mednet_head_dgrad_gn; dW / dbias are summed in another fixed order than mednet_conv3d_wgrad's.
 * mednet_head_dice_bwd with gn_y == NULL and gn_act != MEDNET_ACT_NONE: z is the OUTPUT of a fused conv -> activation layer
 * (UNet3D's last block); dz is stored as (head data gradient) * act'(z), rounded like mednet_act_bwd applied to the stored form. */
int mednet_head_dice_supported(int cin, int cout, int dtype, int label_dtype);
size_t mednet_head_dice_ws_bytes(int n, size_t spatial, int cin, int cout);
int mednet_head_dice_gn_rows(int n, size_t spatial, int cin);
int mednet_head_dice_fwd(const void* z, const void* packed, const float* bias, const void* labels, int label_dtype,
                         int64_t label_stride_n, const float* weight, float* logits, float* loss, float* saved, int n,
                         size_t spatial, int cin, int cout, float eps, int sigmoid, int ignore_index, int z_dtype, void* ws,
                         size_t ws_bytes, mednet_stream stream);
int mednet_head_dice_bwd(const float* logits, const void* labels, int label_dtype, int64_t label_stride_n, const void* packed,
                         const float* weight, const float* saved, const float* dloss, void* dz, const void* gn_y, const void* z,
                         int gn_act, float* gn_partial, float* dw, float* dbias, int n, size_t spatial, int cin, int cout,
                         float eps, int sigmoid, int ignore_index, int z_dtype, void* ws, size_t ws_bytes, mednet_stream stream);
/* mednet_head_dice_bwd (and below the CE and Dice + CE forms) WITHOUT dz: gn_partial, dw and dbias are those of the storing call, bit
 * for bit -- the GroupNorm sums are taken from the values dz would hold -- and nothing else is written; the caller's GroupNorm-3
 * apply pass rebuilds the rows (mednet_gn_act_bwd_fused_res_head, whose _supported says what both take).  gn_y and gn_partial are
 * required; workspace and rows as for the storing call.  Additive to ABI 3. */
int mednet_head_dice_bwd_sums(const float* logits, const void* labels, int label_dtype, int64_t label_stride_n, const void* packed,
                              const float* weight, const float* saved, const float* dloss, const void* gn_y, const void* z,
                              int gn_act, float* gn_partial, float* dw, float* dbias, int n, size_t spatial, int cin, int cout,
                              float eps, int sigmoid, int ignore_index, int z_dtype, void* ws, size_t ws_bytes, mednet_stream stream);

/* The landmark head (LandmarkNet, landmarks.py:66-83: final_conv 32 -> nh heat maps + ncls classes) fused with BOTH terms of its
 * loss (landmarks.py:125-134: sum_c w_c mean f(out_c - heatmap_c), f = square | abs, plus DiceLoss of the class channels,
 * loss.py:114-130) on the matrix cores, 16-bit storage only.  z: N x spatial x cin (NDHWC); heatmaps: uint8, N x nh x spatial,
 * sample stride heatmap_stride_n; labels: uint8, N x spatial, sample stride label_stride_n (both 4-byte aligned per sample);
 * `packed` = the head's mednet_conv3d_pack image (its fp32 [co][ci] block is used, split hi + lo for the MFMAs).
 * _fwd writes class_loss, reg_loss and saved[ncls][2] (the Dice sums the backward needs); the logits only if `logits` != NULL
 * (N x (nh + ncls) x spatial fp32).  _bwd rebuilds the logits with the same instructions, forms their gradient in registers and
 * writes dz (N x spatial x cin), dw [nh + ncls][cin], dbias (nullable) and -- gn_y != NULL -- gn_partial[n][rows][cin][2] =
 * {sum du, sum du * gn_y}, du = dz * act'(z), rows = mednet_head_landmark_gn_rows(spatial), for mednet_gn_act_bwd_fused_res.
 * _supported: cin == 32, 1 <= nh <= 16, 1 <= ncls <= 4, spatial % 4 == 0.  Results equal the unfused launches
 * (mednet_conv3d_fwd k=1, mednet_heatmap_loss_*, mednet_dice_*, mednet_head_dgrad_gn, mednet_conv3d_wgrad k=1) up to fp32
 * summation order. */
int mednet_head_landmark_supported(int cin, int nh, int ncls, int dtype, size_t spatial);
size_t mednet_head_landmark_ws_bytes(int n, size_t spatial, int nh, int ncls);
int mednet_head_landmark_gn_rows(size_t spatial);
int mednet_head_landmark_fwd(const void* z, const void* packed, const float* bias, const void* heatmaps, int64_t heatmap_stride_n,
                             const void* labels, int64_t label_stride_n, const float* class_weight, const float* reg_weight,
                             float* logits, float* class_loss, float* reg_loss, float* saved, int n, size_t spatial, int cin, int nh,
                             int ncls, int kind, float eps, int sigmoid, int ignore_index, int z_dtype, void* ws, size_t ws_bytes,
                             mednet_stream stream);
int mednet_head_landmark_bwd(const void* z, const void* packed, const float* bias, const void* heatmaps, int64_t heatmap_stride_n,
                             const void* labels, int64_t label_stride_n, const float* class_weight, const float* reg_weight,
                             const float* saved, const float* dclass_loss, const float* dreg_loss, void* dz, const void* gn_y,
                             int gn_act, float* gn_partial, float* dw, float* dbias, int n, size_t spatial, int cin, int nh, int ncls,
                             int kind, float eps, int sigmoid, int ignore_index, int z_dtype, void* ws, size_t ws_bytes,
                             mednet_stream stream);
/* The same two heads with nn.CrossEntropyLoss(weight, ignore_index) as the class loss (segmentation.py:49, landmarks.py:49: the
 * callers' `loss='CE'` / `loss_class='CE'`).  Additive to ABI 3: the Dice entry points above are unchanged.
 * mednet_head_ce_*: the segmentation head of mednet_head_dice_* with CE -- same layouts, label forms, workspace, GroupNorm rows
 * and fold rule.  _fwd writes the logits, loss = sum w_y nll / sum w_y over the voxels whose label is not ignore_index, and
 * saved[0] = sum w_y (saved holds 2 floats); a label outside [0, cout) that is not ignore_index makes the loss NaN.  _bwd forms
 * the logit gradient (dloss / saved[0]) w_y (p_k - [k == y]) (0 for ignored voxels) in registers.  Logits, loss, dz and the
 * GroupNorm sums are bit-identical to mednet_conv3d_fwd + mednet_ce_fwd / mednet_ce_bwd (int64 labels) + mednet_head_dgrad_gn;
 * dW / dbias are summed in another fixed order.  _supported: as mednet_head_dice_supported.
 * mednet_head_landmark_cls_*: mednet_head_landmark_* with the class-loss kind as an argument.  MEDNET_CLASS_DICE runs exactly
 * mednet_head_landmark_fwd / _bwd.  MEDNET_CLASS_CE (softmax only: sigmoid must be 0): _fwd writes class_loss = the CE of the
 * class channels (ignore_index honoured, out-of-range labels -> NaN) and saved[0] = sum w_y; _bwd reads saved[0].  dice_metric
 * (nullable, [ncls]): dice_metric(outputs[:, nh:], labels) (loss.py:51-55: softmax, no weight, no mask) from the same pass; with
 * MEDNET_CLASS_DICE it requires sigmoid == 0 and ignore_index == MEDNET_NO_IGNORE.  Workspace: mednet_head_landmark_ws_bytes.
 * MEDNET_CLASS_DICE_CE (sigmoid must be 0 and ignore_index MEDNET_NO_IGNORE, else MEDNET_E_UNSUPPORTED): class_loss = Dice + CE of
 * the class channels with one class-weight vector, as mednet_dice_ce_fwd_lt; saved holds 2 ncls + 1 floats, [ncls][2] = {I, D}
 * followed by sum w_y; dice_metric as with MEDNET_CLASS_DICE.
 * Results equal the unfused launches (mednet_ce_* / mednet_dice_ce_* for the class term) up to fp32 summation order. */
int mednet_head_ce_supported(int cin, int cout, int dtype, int label_dtype);
size_t mednet_head_ce_ws_bytes(int n, size_t spatial, int cin, int cout);
int mednet_head_ce_gn_rows(int n, size_t spatial, int cin);
int mednet_head_ce_fwd(const void* z, const void* packed, const float* bias, const void* labels, int label_dtype,
                       int64_t label_stride_n, const float* weight, float* logits, float* loss, float* saved, int n, size_t spatial,
                       int cin, int cout, int ignore_index, int z_dtype, void* ws, size_t ws_bytes, mednet_stream stream);
int mednet_head_ce_bwd(const float* logits, const void* labels, int label_dtype, int64_t label_stride_n, const void* packed,
                       const float* weight, const float* saved, const float* dloss, void* dz, const void* gn_y, const void* z,
                       int gn_act, float* gn_partial, float* dw, float* dbias, int n, size_t spatial, int cin, int cout,
                       int ignore_index, int z_dtype, void* ws, size_t ws_bytes, mednet_stream stream);
int mednet_head_ce_bwd_sums(const float* logits, const void* labels, int label_dtype, int64_t label_stride_n, const void* packed,
                            const float* weight, const float* saved, const float* dloss, const void* gn_y, const void* z, int gn_act,
                            float* gn_partial, float* dw, float* dbias, int n, size_t spatial, int cin, int cout, int ignore_index,
                            int z_dtype, void* ws, size_t ws_bytes, mednet_stream stream);
/* mednet_head_dice_ce_*: the segmentation head of mednet_head_dice_* (cin in {16, 32, 64}, cout <= 4, f32 / bf16 / f16 features) with
 * the compound class loss DiceLoss(weight, eps) + nn.CrossEntropyLoss(weight) of mednet_dice_ce_fwd_lt.  Additive to ABI 3.  Same
 * arguments, layouts, label forms, GroupNorm rows and fold rule as mednet_head_dice_*; softmax only and no ignore_index: sigmoid != 0
 * or ignore_index != MEDNET_NO_IGNORE is MEDNET_E_UNSUPPORTED.  saved: 2 cout + 1 floats, [cout][2] = {I, D} followed by sum w_y.
 * Workspace: mednet_head_dice_ce_ws_bytes -- the forward writes the Dice rows and the CE rows of every workgroup, so
 * mednet_head_dice_ws_bytes is too small.  A label outside [0, cout) makes the loss and every gradient NaN.
 * Logits, loss, dz and the GroupNorm sums are bit-identical to mednet_conv3d_fwd + mednet_dice_ce_fwd_lt / _bwd_lt +
 * mednet_head_dgrad_gn (hence to the sum of the mednet_dice_* and mednet_ce_* results); dW / dbias are summed in another fixed
 * order, as for mednet_head_dice_bwd. */
int mednet_head_dice_ce_supported(int cin, int cout, int dtype, int label_dtype);
size_t mednet_head_dice_ce_ws_bytes(int n, size_t spatial, int cin, int cout);
int mednet_head_dice_ce_gn_rows(int n, size_t spatial, int cin);
int mednet_head_dice_ce_fwd(const void* z, const void* packed, const float* bias, const void* labels, int label_dtype,
                            int64_t label_stride_n, const float* weight, float* logits, float* loss, float* saved, int n,
                            size_t spatial, int cin, int cout, float eps, int sigmoid, int ignore_index, int z_dtype, void* ws,
                            size_t ws_bytes, mednet_stream stream);
int mednet_head_dice_ce_bwd(const float* logits, const void* labels, int label_dtype, int64_t label_stride_n, const void* packed,
                            const float* weight, const float* saved, const float* dloss, void* dz, const void* gn_y, const void* z,
                            int gn_act, float* gn_partial, float* dw, float* dbias, int n, size_t spatial, int cin, int cout,
                            float eps, int sigmoid, int ignore_index, int z_dtype, void* ws, size_t ws_bytes, mednet_stream stream);
int mednet_head_dice_ce_bwd_sums(const float* logits, const void* labels, int label_dtype, int64_t label_stride_n, const void* packed,
                                 const float* weight, const float* saved, const float* dloss, const void* gn_y, const void* z,
                                 int gn_act, float* gn_partial, float* dw, float* dbias, int n, size_t spatial, int cin, int cout,
                                 float eps, int sigmoid, int ignore_index, int z_dtype, void* ws, size_t ws_bytes, mednet_stream stream);
int mednet_head_landmark_cls_fwd(const void* z, const void* packed, const float* bias, const void* heatmaps, int64_t heatmap_stride_n,
                                 const void* labels, int64_t label_stride_n, const float* class_weight, const float* reg_weight,
                                 float* logits, float* class_loss, float* reg_loss, float* saved, float* dice_metric, int n,
                                 size_t spatial, int cin, int nh, int ncls, int kind, int class_kind, float eps, int sigmoid,
                                 int ignore_index, int z_dtype, void* ws, size_t ws_bytes, mednet_stream stream);
int mednet_head_landmark_cls_bwd(const void* z, const void* packed, const float* bias, const void* heatmaps, int64_t heatmap_stride_n,
                                 const void* labels, int64_t label_stride_n, const float* class_weight, const float* reg_weight,
                                 const float* saved, const float* dclass_loss, const float* dreg_loss, void* dz, const void* gn_y,
                                 int gn_act, float* gn_partial, float* dw, float* dbias, int n, size_t spatial, int cin, int nh,
                                 int ncls, int kind, int class_kind, float eps, int sigmoid, int ignore_index, int z_dtype, void* ws,
                                 size_t ws_bytes, mednet_stream stream);
/* The segmentation head for 5 .. 16 classes (SegmentationNet, segmentation.py:30-31, 58-62: final_conv 32 -> ncls) fused with its
 * loss on the matrix cores, 16-bit storage only.  Additive to ABI 3; mednet_head_dice_* / mednet_head_ce_* (<= 4 classes) are
 * unchanged.  class_kind MEDNET_CLASS_DICE: DiceLoss (loss.py:114-130: class weight in the numerator, eps, sigmoid | softmax,
 * ignore_index on the one-hot target); MEDNET_CLASS_CE: nn.CrossEntropyLoss(weight, ignore_index) (softmax: sigmoid must be 0);
 * MEDNET_CLASS_DICE_CE: their sum with one class-weight vector, as mednet_dice_ce_fwd_lt (sigmoid must be 0 and ignore_index
 * MEDNET_NO_IGNORE, else MEDNET_E_UNSUPPORTED; saved holds 2 ncls + 1 floats: [ncls][2] = {I, D}, then sum w_y; the workspace
 * query already covers the Dice rows plus the CE rows).
 * z: N x spatial x cin (NDHWC); labels: MEDNET_U8, N x spatial, sample stride label_stride_n, base pointer and stride multiples
 * of 4 bytes; `packed` = the head's mednet_conv3d_pack image (its fp32 [co][ci] block, split hi + lo for the MFMAs).
 * _fwd writes loss and saved (Dice: [ncls][2] = {I, D}; CE: saved[0] = sum w_y, saved holds 2 floats), both required, and the
 * logits (N x ncls x spatial fp32, planar) only if `logits` != NULL.
 * A label >= ncls that is not ignore_index makes the loss NaN.
 * _bwd rebuilds the logits with the same instructions, forms their gradient in registers (closed forms of mednet_dice_bwd /
 * mednet_ce_bwd) and writes dz (N x spatial x cin, storage type), dw [ncls][cin], dbias (nullable) and -- gn_y and gn_partial,
 * which go together -- gn_partial[n][rows][cin][2] = {sum du, sum du * gn_y}, du = dz * act'(z), rows =
 * mednet_head_seg_gn_rows(spatial) = ceil(ceil(spatial / 128) / 64), for mednet_gn_act_bwd_fused_res.
 * Workspace: mednet_head_seg_ws_bytes(n, spatial, ncls) for both calls (n * rows rows of 32 * 33 floats in the backward).
 * _supported: cin == 32, 5 <= ncls <= 16, dtype MEDNET_BF16 | MEDNET_F16, label_dtype MEDNET_U8, spatial % 4 == 0, tuning option
 * head_seg_mfma != 0.  Results equal the unfused launches (mednet_conv3d_fwd k=1, mednet_dice_* / mednet_ce_*,
 * mednet_head_dgrad_gn, mednet_conv3d_wgrad k=1) up to fp32 summation order; every sum is made in a fixed order. */
int mednet_head_seg_supported(int cin, int ncls, int dtype, int label_dtype, size_t spatial);
size_t mednet_head_seg_ws_bytes(int n, size_t spatial, int ncls);
int mednet_head_seg_gn_rows(size_t spatial);
int mednet_head_seg_fwd(const void* z, const void* packed, const float* bias, const void* labels, int64_t label_stride_n,
                        const float* class_weight, float* logits, float* loss, float* saved, int n, size_t spatial, int cin,
                        int ncls, int class_kind, float eps, int sigmoid, int ignore_index, int z_dtype, void* ws, size_t ws_bytes,
                        mednet_stream stream);
int mednet_head_seg_bwd(const void* z, const void* packed, const float* bias, const void* labels, int64_t label_stride_n,
                        const float* class_weight, const float* saved, const float* dloss, void* dz, const void* gn_y, int gn_act,
                        float* gn_partial, float* dw, float* dbias, int n, size_t spatial, int cin, int ncls, int class_kind,
                        float eps, int sigmoid, int ignore_index, int z_dtype, void* ws, size_t ws_bytes, mednet_stream stream);
/* Deep supervision: the auxiliary 1x1x1 head on a coarser decoder level fused with its class loss and with the junction "block
 * output -> {next decoder, auxiliary head}".  Additive to ABI 3.  z: N x (d h w) x cin (NDHWC), the level's block output; labels: the
 * FULL-resolution MEDNET_U8 volume N x D x H x W (sample stride label_stride_n, any alignment), of which voxel (z, y, x) of the level
 * reads [z << shift][y << shift][x << shift] -- F.interpolate(mode="nearest") for the scale 2^-shift; d == D >> shift (h, w alike,
 * else MEDNET_E_SHAPE), shift in 1 .. 3.  class_kind, eps, sigmoid, ignore_index, class_weight, packed, loss and saved as
 * mednet_head_seg_*.  _bwd writes dz = round(W^T dl + d_pass) -- d_pass (nullable, N x (d h w) x cin, storage type) is the gradient
 * the level's other consumer sent, added in fp32 before the one rounding --, dw [ncls][cin] and dbias (nullable).  gn_y / gn_partial go
 * together (else MEDNET_E_SHAPE) and are accepted only when mednet_ds_head_gn_rows(...) > 0; it answers 0 in this version (the
 * GroupNorm-3 sums of the producing block are not taken here), so both must be NULL (else MEDNET_E_UNSUPPORTED).
 * _supported: cin in 64, 96, .., 256, 1 <= ncls <= 16, dtype MEDNET_BF16 | MEDNET_F16, label_dtype MEDNET_U8, d h w % 4 == 0,
 * shift in 1 .. 3, tuning option ds_head_fuse != 0.  Workspace: mednet_ds_head_ws_bytes for both calls.  Every sum is made in a fixed
 * order (no atomics): results are bitwise repeatable. */
int mednet_ds_head_supported(int cin, int ncls, int dtype, int label_dtype, int d, int h, int w, int shift);
size_t mednet_ds_head_ws_bytes(int n, int d, int h, int w, int cin, int ncls);
int mednet_ds_head_gn_rows(int d, int h, int w, int cin, int dtype);
int mednet_ds_head_fwd(const void* z, const void* packed, const float* bias, const void* labels, int label_dtype,
                       int64_t label_stride_n, const float* class_weight, float* loss, float* saved, int n, int d, int h, int w, int D,
                       int H, int W, int shift, int cin, int ncls, int class_kind, float eps, int sigmoid, int ignore_index, int z_dtype,
                       void* ws, size_t ws_bytes, mednet_stream stream);
int mednet_ds_head_bwd(const void* z, const void* packed, const float* bias, const void* labels, int label_dtype,
                       int64_t label_stride_n, const float* class_weight, const float* saved, const float* dloss, const void* d_pass,
                       void* dz, const void* gn_y, int gn_act, float* gn_partial, float* dw, float* dbias, int n, int d, int h, int w,
                       int D, int H, int W, int shift, int cin, int ncls, int class_kind, float eps, int sigmoid, int ignore_index,
                       int z_dtype, void* ws, size_t ws_bytes, mednet_stream stream);
/* nn.CrossEntropyLoss(weight)  segmentation.py:49: sum w_y * -log softmax_y / sum w_y.  saved[0] = sum w_y. */
int mednet_ce_fwd(const float* logits, const int64_t* labels, const float* weight, float* loss, float* saved,
                  int n, int c, size_t spatial, int64_t stride_n, int64_t stride_c, int ignore_index, void* ws,
                  size_t ws_bytes, mednet_stream stream);
int mednet_ce_bwd(const float* logits, const int64_t* labels, const float* weight, const float* saved,
                  const float* dloss, float* dlogits, int n, int c, size_t spatial, int64_t stride_n,
                  int64_t stride_c, int ignore_index, mednet_stream stream);
/* LandmarkNet.loss regression term  landmarks.py:129-132: sum_c w_c * mean_{n,v} f(out[:,c]-hm[:,c]),
 * f = square (L2) | abs (L1).  target is fp32 or uint8 (tgt_u8=1), contiguous N x C x spatial. */
int mednet_heatmap_loss_fwd(const float* out, const void* target, const float* cweight, float* loss, int n, int c,
                            size_t spatial, int64_t stride_n, int64_t stride_c, int kind, int tgt_u8, void* ws,
                            size_t ws_bytes, mednet_stream stream);
/* (dout: the layout of `out`, as dlogits above) */
int mednet_heatmap_loss_bwd(const float* out, const void* target, const float* cweight, const float* dloss,
                            float* dout, int n, int c, size_t spatial, int64_t stride_n, int64_t stride_c, int kind,
                            int tgt_u8, mednet_stream stream);
/* ... with an element stride between the samples of `target` (channel ch of sample n at + n * target_stride_n + ch * spatial): the
 * heat-map channels of a label volume (`batch['label'][:, :-1]`, landmarks.py:68) are consumed where they lie, no copy. */
int mednet_heatmap_loss_fwd_strided(const float* out, const void* target, int64_t target_stride_n, const float* cweight, float* loss,
                                    int n, int c, size_t spatial, int64_t stride_n, int64_t stride_c, int kind, int tgt_u8, void* ws,
                                    size_t ws_bytes, mednet_stream stream);
int mednet_heatmap_loss_bwd_strided(const float* out, const void* target, int64_t target_stride_n, const float* cweight,
                                    const float* dloss, float* dout, int n, int c, size_t spatial, int64_t stride_n,
                                    int64_t stride_c, int kind, int tgt_u8, mednet_stream stream);

/* ---- torch.optim.Adam(lr) step  segmentation.py:119-120 (betas .9/.999, eps 1e-8, wd 0), flat fp32 buffers (csrc/optim.hip) --- */
int mednet_adam_step(float* p, const float* g, float* m, float* v, size_t count, float lr, float beta1,
                     float beta2, float eps, float weight_decay, int step, float grad_scale,
                     mednet_stream stream);
/* fp16 storage (BASELINE config 5): the same update behind dynamic loss scaling, with no host synchronisation.
 * scaler_state (device, 4 floats) = {scale, good steps since the last change, optimizer steps taken, found_inf}; the caller
 * multiplies the loss by scaler_state[0] on the device.  Three launches: raise found_inf if any gradient is NaN/inf; Adam
 * on g / (scale * world) with the device-side step count, skipped entirely when found_inf; then the scale is multiplied
 * by backoff_factor (overflow) or a good step is counted and every growth_interval of them multiply it by growth_factor
 * (torch.cuda.amp.GradScaler's rule; the reference itself trains fp32, train_seg.py:127 has precision=16 commented out). */
int mednet_adam_step_scaled(float* p, const float* g, float* m, float* v, size_t count, float lr, float beta1, float beta2,
                            float eps, float weight_decay, float inv_world, float* scaler_state, float growth_factor,
                            float backoff_factor, int growth_interval, mednet_stream stream);

/* ---- optimisers behind a global gradient norm (additive to ABI 3; the reference trains with plain Adam only) ---------------------
 * Optimiser state opt_state (device, 8 floats): {sumsq, norm, coef, nonfinite, steps taken, steps skipped, -, -}; a fresh one is
 * {0, 0, 1, 0, 0, 0, 0, 0}.  scaler_state is mednet_adam_step_scaled's loss-scaler state or NULL.  In every entry
 *   gscale = scaler_state ? inv_world / scaler_state[0] : inv_world                                       (fp32, on the device)
 *
 * mednet_grad_norm: two launches, no atomics, bitwise reproducible (the grid is a function of count alone).
 *   partial[row] = sum over the row's elements of (g * gscale)^2     fp32, fmaf(s, s, acc), s = g * gscale: scaled BEFORE squaring
 *   sum          = the partials added in a fixed order in fp64
 *   sumsq = (float)sum;  norm = (float)sqrt(sum);  coef = max_norm > 0 ? (float)min(1, max_norm / (sqrt(sum) + 1e-6)) : 1
 *   nonfinite = sumsq is NaN or inf          every NaN / +-inf gradient, and a finite one whose scaled square overflows fp32: that
 *                                            step is skipped as well.  With a scaler state, found_inf (entry 3) is raised too, so this
 *                                            pass replaces the overflow sweep of mednet_adam_step_scaled.
 * coef is torch.nn.utils.clip_grad_norm_'s clip coefficient; max_norm == 0 turns clipping off.  g: any 4-byte aligned pointer, any
 * count >= 1.  ws holds one float per row: mednet_grad_norm_ws_bytes(count) / 4 rows (0 for count == 0). */
size_t mednet_grad_norm_ws_bytes(size_t count);
int mednet_grad_norm(const float* g, size_t count, float inv_world, float* scaler_state, float max_norm, float* opt_state, void* ws,
                     size_t ws_bytes, mednet_stream stream);
/* torch.optim.SGD(lr, momentum, dampening 0, weight_decay, nesterov) on flat fp32 buffers, per element, fp32:
 *   skipped entirely when nonfinite (or the scaler's found_inf) is set: p, buf and the step count stay bit-unchanged
 *   gr  = (g * gscale) * coef
 *   gr  = fma(wd, p, gr)                        when wd != 0
 *   buf = fma(mu, buf, gr)                      when mu != 0 (a zero-initialised buffer reproduces torch's first step)
 *   d   = nesterov ? fma(mu, buf, gr) : buf     (d = gr when mu == 0: buf may be NULL and is not touched)
 *   p   = fma(-lr, d, p)
 * then one thread applies the loss scaler's update rule (scaler_state given) or counts the step in opt_state[4] / a skipped one in
 * opt_state[5], and clears nonfinite.  opt_state == NULL (only without a scaler state): coef = 1, no guard, one launch. */
int mednet_sgd_step(float* p, const float* g, float* buf, size_t count, float lr, float momentum, int nesterov, float weight_decay,
                    float inv_world, float* opt_state, float* scaler_state, float growth_factor, float backoff_factor,
                    int growth_interval, mednet_stream stream);
/* torch.optim.Adam (decoupled == 0) / torch.optim.AdamW (decoupled != 0) behind the norm pass, per element, fp32:
 *   skipped entirely when nonfinite (or found_inf) is set: p, m, v and the step count stay bit-unchanged
 *   t   = (scaler_state ? scaler_state[2] : opt_state[4]) + 1;  bc1 = 1 - beta1^t;  bc2s = sqrt(1 - beta2^t)
 *   gr  = (g * gscale) * coef
 *   Adam:  gr = fma(wd, p, gr)                  AdamW:  p = p * (1 - lr * wd)                   (each when wd != 0)
 *   m   = beta1 * m + (1 - beta1) * gr;  v = beta2 * v + (1 - beta2) * gr * gr
 *   p   = p - (lr / bc1) * (m / (sqrt(v) / bc2s + eps))
 * (the one statement of these lines, adam_lines in csrc/optim.hip, serves mednet_adam_step and mednet_adam_step_scaled with coef == 1:
 * with decoupled == 0 the scaled entry and this one give the same bits), then the state update as above. */
int mednet_adamw_step(float* p, const float* g, float* m, float* v, size_t count, float lr, float beta1, float beta2, float eps,
                      float weight_decay, int decoupled, float inv_world, float* opt_state, float* scaler_state, float growth_factor,
                      float backoff_factor, int growth_interval, mednet_stream stream);

/* ---- inference path ------------------------------------------------------------------------ */
enum { MEDNET_PAD_CONSTANT = 0, MEDNET_PAD_SYMMETRIC = 1 };
/* midasmednet/dataset.py:349-390 (grid_patch_generator): patch b = padded(volume)[:, pos[b] : pos[b] + patch] where the
 * volume (C x D x H x W, fp32) is padded by the overlap in front (np.pad constant-0 or symmetric); pos = B x 3 int32 grid
 * positions on the device.  out: B x C x pD x pH x pW fp32 (what predict.py:85 feeds the network). */
int mednet_grid_gather(const float* volume, const int* pos, float* out, int batch, int c, int d, int h, int w, int pd,
                       int ph, int pw, int ov0, int ov1, int ov2, int pad_mode, mednet_stream stream);
/* examples/predict.py:88-95 + GridPatchSampler.add_processed_batch (dataset.py:446-474) in one pass: logits B x (H +
 * classes) x pD x pH x pW (planar fp32) -> result (H + 1) x D x H x W uint8 (heat maps clipped to 0..255 and truncated,
 * then the arg-max class); only the crop window [crop_start, crop_start + crop_shape) of each patch is written, at
 * pos[b] + offset, and what hangs over the volume is dropped.  The caller derives the window from the reference's slicing
 * (`data[:, o0:-o1, o1:-o1, o2:-o2]`, dataset.py:452-455). */
int mednet_predict_assemble(const float* logits, const int* pos, uint8_t* result, int batch, int num_heatmaps,
                            int num_classes, int d, int h, int w, int pd, int ph, int pw, int crop_start0, int crop_start1,
                            int crop_start2, int crop_d, int crop_h, int crop_w, mednet_stream stream);

/* ---- blended sliding-window inference (additive to ABI 3; the reference has no counterpart: its stitch is the crop above) ------
 * Overlapping patches are blended with a separable importance window instead of being cropped: every patch adds
 * window-weighted class probabilities (or logits) and heat maps to fp32 accumulators over the whole volume, and a last pass divides
 * by the accumulated weight.  No atomics: the same patches in the same order give the same bits, whatever the batch size.
 *
 * mednet_grid_gather_mirror: mednet_grid_gather with test-time mirroring.  Bit k of `mirror` (0..7) reverses patch axis k: the patch
 * voxel (z, y, x) holds what the unmirrored patch holds at (pD - 1 - z, ..) on the flagged axes.  mirror == 0 is mednet_grid_gather
 * bit for bit (one kernel serves both entries).  Another mask is MEDNET_E_UNSUPPORTED. */
int mednet_grid_gather_mirror(const float* volume, const int* pos, float* out, int batch, int c, int d, int h, int w, int pd,
                              int ph, int pw, int ov0, int ov1, int ov2, int pad_mode, int mirror, mednet_stream stream);
/* logits: batch x (H + classes) x pD x pH x pW planar fp32, as the model returns it; pos: the rows mednet_grid_gather takes (patch b
 * covers the volume voxels [pos[b] - ov, pos[b] - ov + patch); what lies outside the volume -- the padding in front, the overhang
 * behind -- is dropped).  win0..2: fp32 tables (device) of pD, pH, pW entries; a voxel's weight is (win0[z] * win1[y]) * win2[x] in
 * fp32, in that association.  acc ((H + classes) x D x H x W fp32) and wsum (D x H x W fp32) are read-modify-write; zero them before
 * the first patch.  Heat-map channels add weight * value; class channels add weight * softmax(logits)_c with
 * MEDNET_BLEND_PROBABILITIES (one softmax per voxel per patch: max-subtracted, expf, one reciprocal) or weight * logit_c with
 * MEDNET_BLEND_LOGITS; each addition is one fmaf.  Another class_mode is MEDNET_E_UNSUPPORTED.
 * mirror (0..7): the logits belong to a patch gathered with that mask and are read at the reversed index on the flagged axes -- the
 * flip back.  The WEIGHT is looked up at the unmirrored patch coordinate, i.e. the window is fixed to the volume, not to the
 * mirrored patch; this only matters for an asymmetric custom window.
 * Rows of one launch may overlap: a voxel is owned by the first row of the launch that holds it, whose thread adds the contributions
 * of all the launch's rows in row order; across launches stream order continues that order.  batch <= 65535. */
enum { MEDNET_BLEND_PROBABILITIES = 0, MEDNET_BLEND_LOGITS = 1 };
int mednet_blend_accumulate(const float* logits, const int* pos, float* acc, float* wsum, const float* win0, const float* win1,
                            const float* win2, int batch, int num_heatmaps, int num_classes, int d, int h, int w, int pd, int ph,
                            int pw, int ov0, int ov1, int ov2, int mirror, int class_mode, mednet_stream stream);
/* One pass over the voxels.  Any of the three outputs may be NULL (all three: MEDNET_E_SHAPE).
 *   heat      H x D x H x W fp32            acc[k] / wsum
 *   prob      classes x D x H x W           acc[H + c] / wsum (MEDNET_BLEND_PROBABILITIES) or softmax over c of acc[H + c] / wsum
 *                                           (MEDNET_BLEND_LOGITS); prob_dtype MEDNET_F32 or MEDNET_F16 (rounded once), else MEDNET_E_DTYPE
 *   result_u8 (H + 1) x D x H x W uint8     mednet_predict_assemble's layout: (uint8)(int)clamp(heat, 0, 255), then the arg-max of the
 *                                           class accumulators, first maximum on ties
 * A voxel whose wsum is 0 (none with grid_positions' grid) reads 0 everywhere, not NaN. */
int mednet_blend_finalize(const float* acc, const float* wsum, uint8_t* result_u8, void* prob, int prob_dtype, float* heat,
                          int num_heatmaps, int num_classes, int d, int h, int w, int class_mode, mednet_stream stream);
/* Landmark positions: per channel of heat (H x voxels fp32) the maximum (out_value, fp32 H) and its flat index (out_index, int64 H),
 * the lowest index on ties.  A NaN never wins; a channel of NaNs only gives index -1 and value -inf.  Two deterministic stages: one
 * partial per workgroup of 4096 voxels in ws, then one workgroup per channel.  A ws smaller than _ws_bytes is MEDNET_E_WORKSPACE; ws
 * is 8-byte aligned. */
size_t mednet_heatmap_peaks_ws_bytes(int num_heatmaps, size_t voxels);
int mednet_heatmap_peaks(const float* heat, int num_heatmaps, size_t voxels, int64_t* out_index, float* out_value, void* ws,
                         size_t ws_bytes, mednet_stream stream);

/* ---- training-patch sampler ------------------------------------------------------------------ */
/* MedDataset.__getitem__'s crop + cast (dataset.py:313-331) from a device-resident volume src (C x D x H x W; f16 / f32
 * images, u8 labels or heat maps): for i < count,
 *   out[slot[i]][c_off + c][z][y][x] = cast(src[c][pos[i][0] + z][pos[i][1] + y][pos[i][2] + x])
 * out: B x c_total x pD x pH x pW (f32 for images, u8 for labels); pos (count x 3) and slot (count) are int32 on the device.
 * Positions come from the host-side restatement of the reference's sampling (same numpy generator calls). */
int mednet_crop_patches(const void* src, int src_dtype, const int* pos, const int* slot, int count, void* out, int dst_dtype,
                        int c, int d, int h, int w, int c_total, int c_off, int pd, int ph, int pw, mednet_stream stream);
/* ---- intensity augmentation of a batch of cropped patches, in place: the Compose of examples/train_seg.py:82-86
 * (batchgenerators BrightnessTransform -> GammaTransform -> ContrastAugmentationTransform, applied per sample at
 * dataset.py:340-341).  data: batch x channels x spatial fp32; params[batch][channels][3] (device) = {additive brightness,
 * gamma, contrast factor} drawn by the caller in batchgenerators' order (mednet_hip.sampler.draw_augmentation); the
 * data-dependent parts (sample range for the gamma map, channel mean / range for the contrast step) are computed on the
 * device: five launches, no synchronisation. */
size_t mednet_augment_ws_bytes(int batch, int channels, size_t spatial);
int mednet_augment_patches(float* data, const float* params, int batch, int channels, size_t spatial, void* ws,
                           size_t ws_bytes, mednet_stream stream);

/* ---- spatial augmentation of training patches (additive to ABI 3): crop + rotation / scale / mirror + elastic deformation in one
 * pass over a device-resident volume, the `transform=` slot of the reference (midasmednet/dataset.py:223,340-341) for the spatial
 * transforms.  One call per source volume, as mednet_crop_patches: src is C x D x H x W, out is B x c_total x pD x pH x pW and row
 * i < count writes channels [c_off, c_off + c) of sample slot[i].  Pairs: f16 -> f32 and f32 -> f32 (images), u8 -> u8 (heat maps:
 * MEDNET_INTERP_LINEAR, rounded once to nearest-even; labels: MEDNET_INTERP_NEAREST); every pair takes either interpolation, another
 * pair is MEDNET_E_DTYPE.
 *   affine  count x 12 fp32 (device): row-major 3 x 4 [A | t] per row, built by the host.
 *   disp    NULL, or count x 3 x gd x gh x gw fp32 (device): a coarse control lattice of displacements in PATCH voxels (component 0
 *           along z, 1 along y, 2 along x) whose corner points sit on the patch's corner voxels.
 * For output voxel (z, y, x) -- all fp32, in exactly this association:
 *   1. u = (z - (pD - 1)/2, y - (pH - 1)/2, x - (pW - 1)/2)                 (half-integer centres: exact)
 *   2. with disp: lattice coordinate g_k = fl(idx_k * r_k), r_k = fl((extent_k - 1) / (p_k - 1)) (0 if p_k == 1), cell
 *      min(floor(g_k), extent_k - 2), weight g_k - cell; each component is lerped over x, then y, then z as fmaf(q, b - a, a) and
 *      added: u_j = fl(u_j + D_j)
 *   3. s_k = fmaf(A[k][0], u_0, fmaf(A[k][1], u_1, fmaf(A[k][2], u_2, t[k])))    (source coordinate, volume voxels)
 *   4. linear: cell f = floor(s), weights s - f, lerp over x, then y, then z as fmaf(w, b - a, a) (weight 0 returns a bit for bit);
 *      nearest: index floor(s + 0.5f)
 *   5. border, per call: MEDNET_BORDER_CONSTANT -- a tap outside the volume reads cval and the result is still interpolated towards it
 *      (scipy.ndimage 'grid-constant'); MEDNET_BORDER_EDGE -- tap indices are clamped (scipy.ndimage 'nearest').  cval is converted
 *      to the output type as a value of the source would be.
 * Any coordinate is safe -- NaN, +-inf, |s| >= 2^31: it is clamped in float to [-2, n + 1] before the conversion and NaN counts as
 * outside (csrc/warp_index.h).  Unlike the crop, the patch may be larger than the volume: the border rule covers it.
 * Refused before anything is launched: a null src / affine / slot / out, count <= 0, a non-positive extent, c_off + c > c_total, disp
 * with a lattice extent < 2, count > 65535, a volume, patch or lattice extent above 2^24 - 2 (MEDNET_E_SHAPE); an unknown interp or border, and
 * for the u8 pair a cval outside [0, 255] or NaN -- it could not be converted to a byte -- (MEDNET_E_UNSUPPORTED); another dtype pair
 * (MEDNET_E_DTYPE). */
enum { MEDNET_INTERP_LINEAR = 0, MEDNET_INTERP_NEAREST = 1 };
enum { MEDNET_BORDER_CONSTANT = 0, MEDNET_BORDER_EDGE = 1 };
int mednet_warp_patches(const void* src, int src_dtype, const float* affine, const float* disp, int gd, int gh, int gw,
                        const int* slot, int count, void* out, int dst_dtype, int c, int d, int h, int w, int c_total, int c_off,
                        int pd, int ph, int pw, int interp, int border, float cval, mednet_stream stream);

/* ---- validation sample logging: the arrays `log_samples` (segmentation.py:67-92, landmarks.py:85-123) hands
 * to imshow through vis_loglabels / vis_logheatmaps (utils/plots.py:45-127), from ONE sample where its tensors lie.  Additive to
 * ABI 3.  All pointers address that sample: logits = channel 0 of its network output (planar fp32, plane k at + k * stride_c
 * elements: the num_heatmaps raw heat-map outputs, then num_classes class planes), labels = its class map (MEDNET_U8 or
 * MEDNET_I64, d*h*w dense -- the last channel of a label volume is read in place), heatmaps = its num_heatmaps target planes
 * (MEDNET_U8 or MEDNET_F32, dense), input = its first input channel.  `axis` (0, 1, 2) counts within d x h x w and is reduced
 * away; a panel is the remaining two extents, row-major:
 *   pred_mip            uint8          max over the axis of the arg-max over the class planes (first maximum on ties, like
 *                                      torch.argmax; the reference's soft-max does not change it), 1 <= num_classes <= 256
 *   label_mip           uint8          max over the axis of the class map (values above 255 are a caller error: they wrap)
 *   input_mip           fp32           MEDNET_MIP_MEAN: mean, MEDNET_MIP_MAX: max over the axis of the input
 *   heatmap_mip         fp32 [nh][..]  max over the axis of the target heat maps
 *   output_heatmap_mip  fp32 [nh][..]  max over the axis of the raw heat-map outputs (landmarks.py:94 does not clip them)
 * A NULL output pointer switches its panel off (its source is then not read and may be NULL); num_heatmaps == 0 switches both
 * heat-map panels off.  Each source is read once -- the class planes once for arg-max and projection together -- and nothing
 * intermediate is stored.  Axes 0 and 1 cut the reduced extent into segments (partials in `ws`, combined in index order by a
 * second launch); axis 2 reduces inside a wave and needs no workspace (_ws_bytes returns 0).  No atomics: the same inputs give the
 * same bits.  max ignores NaN (fmaxf). */
enum { MEDNET_MIP_MEAN = 0, MEDNET_MIP_MAX = 1 };
size_t mednet_sample_panels_ws_bytes(int d, int h, int w, int num_heatmaps, int axis);
int mednet_sample_panels(const float* logits, int64_t stride_c, int num_heatmaps, int num_classes, const void* labels,
                         int label_dtype, const void* heatmaps, int heatmap_dtype, const float* input, uint8_t* pred_mip,
                         uint8_t* label_mip, float* input_mip, float* heatmap_mip, float* output_heatmap_mip, int d, int h, int w,
                         int axis, int image_mode, void* ws, size_t ws_bytes, mednet_stream stream);

/* ---- case-level evaluation of a whole-volume prediction (additive to ABI 3; the reference has no evaluation code) -----------------
 * Volumes are dense d x h x w, every extent in 1 .. 2048 (else MEDNET_E_SHAPE).  No float atomics: partial rows per workgroup in the
 * caller's workspace, then a finalize launch; every grid is a function of the extents alone, so the same inputs give the same bits.
 * Every refusal -- a null pointer, an extent outside 1 .. 2048, ncls outside 1 .. 32, a spacing that is not finite and positive, a
 * negative or NaN tolerance, an undersized workspace -- returns its code before anything is launched.
 *
 * mednet_confusion: pred, label uint8 (any address); counts int64 [ncls * ncls + 1] (8-byte aligned):
 *   counts[l * ncls + p]  voxels with label l predicted as p
 *   counts[ncls * ncls]   voxels left out because label or prediction is >= ncls
 * A voxel whose label equals ignore_index is counted nowhere (MEDNET_NO_IGNORE: none).  ncls > 32 is MEDNET_E_UNSUPPORTED.  Workspace:
 * one row of ncls * ncls + 1 uint32 per workgroup, ceil(voxels / 4096) workgroups up to 2048 (4-byte aligned). */
size_t mednet_confusion_ws_bytes(int d, int h, int w, int ncls);
int mednet_confusion(const uint8_t* pred, const uint8_t* label, int d, int h, int w, int ncls, int ignore_index, int64_t* counts,
                     void* ws, size_t ws_bytes, mednet_stream stream);
/* out[v] = 1 where vol[v] == cls and one of the six face neighbours is != cls or lies outside the volume, else 0: mask & ~erosion
 * with the 6-connected structuring element and background outside (scipy.ndimage.binary_erosion's default border).  vol2 / out2: a
 * second volume of the same extents in the same launch (prediction and label together), or both NULL.  cls in 0 .. 255. */
int mednet_surface_mask(const uint8_t* vol, uint8_t* out, const uint8_t* vol2, uint8_t* out2, int cls, int d, int h, int w,
                        mednet_stream stream);
/* Exact squared Euclidean distance transform: seed uint8 (nonzero = seed), out fp32,
 *   out[v] = min over seeds s of  sum over the axes a of (spacing_a * (v_a - s_a))^2        (+inf everywhere without a seed)
 * Separable, three launches (x, y, z) in place on `out`, no workspace.  The arithmetic, fixed so that a test can be exact:
 *   T_a(k)    = fl32((spacing_a * k)^2)           formed in fp64 from the fp32 spacing, k an integer index difference: ONE rounding
 *   a pass    : out[i] = min over ALL j of the line of  fl32(g[j] + T_a(i - j)),  g = 0 / +inf from the seeds in the x pass, the
 *               previous pass's output after it; nothing is reassociated across axes
 * With unit or dyadic spacing every operand is a multiple of a power of two below 2^24 (3 * 2047^2 < 2^24) and the result is exact.
 * In general every term is non-negative and the x term sees three roundings, the y term three, the z term two: the result is within
 * (1 + 2^-24)^3 - 1 of the real minimum.  A workgroup stages a bundle of 64 / 32 / 16 neighbouring lines in LDS (extent up to 240 /
 * 464 / 2048; at most 152 KiB), so the y and z passes read and write whole runs of x. */
int mednet_edt_sq(const uint8_t* seed, float* out, int d, int h, int w, float sz, float sy, float sx, mednet_stream stream);
/* Over the voxels with surf != 0 (surf uint8, d2 fp32, as mednet_surface_mask and mednet_edt_sq write them):
 *   counts[0] = their number;  counts[1] = those with d2 <= tol_sq                                               (int64, 8-byte aligned)
 *   *max_d2   = the largest d2, -inf for an empty surface                                                        (fp32)
 *   *sum_sqrt = sum of the correctly rounded fp32 roots sqrtf(d2), added in fp64 from the first add on, fixed order   (fp64)
 * A +inf in d2 reaches max and sum and is not within any tolerance.  Workspace: 28 bytes per workgroup (8-byte aligned). */
size_t mednet_surface_stats_ws_bytes(int d, int h, int w);
int mednet_surface_stats(const uint8_t* surf, const float* d2, int d, int h, int w, float tol_sq, int64_t* counts, float* max_d2,
                         double* sum_sqrt, void* ws, size_t ws_bytes, mednet_stream stream);

/* ---- connected components of a uint8 volume (additive to ABI 3; the reference has no post-processing code) ---------------------------
 * Volumes are dense d x h x w uint8 at any byte address, every extent in 1 .. 2048 and d * h * w < 2^31 (else MEDNET_E_SHAPE), so a
 * linear voxel index fits an int32.  Integer atomics only: every result is a pure function of the input, bit for bit.  Every refusal
 * -- a null pointer, the extents, a cls outside 0 .. 255 / MEDNET_CC_ALL, invert with MEDNET_CC_ALL, a misaligned labels / table /
 * info, k < 0, fill outside 0 .. 255 (all MEDNET_E_SHAPE), a connectivity other than 6 / 18 / 26 (MEDNET_E_UNSUPPORTED), an undersized
 * workspace (MEDNET_E_WORKSPACE) -- returns its code before anything is launched.
 *
 * mednet_cc_label: foreground = voxels with vol == cls (cls in 0 .. 255), with invert = 1 those with vol != cls; cls = MEDNET_CC_ALL
 * (invert must be 0): every non-zero voxel, two voxels being connected only if their values are equal -- one labelling for all classes.
 * connectivity 6, 18, 26: neighbours that differ in at most 1, 2, 3 coordinates by 1 (scipy's generate_binary_structure(3, 1 | 2 | 3)).
 *   labels  int32 d x h x w (4-byte aligned): 0 on background, 1 .. K on foreground; components are numbered in raster order (z, y, x;
 *           x fastest) of their first voxel, which is scipy.ndimage.label's numbering.  The volume holds the parents while the call runs.
 *   info    int64 [2] (8-byte aligned): info[0] = K; info[1] = 0, or non-zero if a parent walk reached its step cap (the voxel count;
 *           unreachable unless the kernel is wrong -- labels are then not to be used)
 * Workspace: one uint32 per numbering row, ceil(voxels / 4096) rows up to 2048 (4-byte aligned); 0 for illegal extents. */
#define MEDNET_CC_ALL (-1)
size_t mednet_cc_ws_bytes(int d, int h, int w);
int mednet_cc_label(const uint8_t* vol, int cls, int invert, int connectivity, int d, int h, int w, int32_t* labels, int64_t* info,
                    void* ws, size_t ws_bytes, mednet_stream stream);
/* table int64 [k][11] (8-byte aligned; may be uninitialised, NULL only with k = 0), row id - 1 for component id of `labels`:
 *   voxel count, zmin, zmax, ymin, ymax, xmin, xmax, sum of z, sum of y, sum of x, the component's value in vol
 * k = 0 launches nothing.  Labels above k are left out. */
int mednet_cc_stats(const uint8_t* vol, const int32_t* labels, int d, int h, int w, int64_t k, int64_t* table, mednet_stream stream);
/* out[v] = (labels[v] > 0 && !keep[labels[v]]) ? fill : vol[v];  keep uint8 [K + 1], entry 0 is ignored; out == vol is legal. */
int mednet_cc_select(const uint8_t* vol, const int32_t* labels, const uint8_t* keep, int fill, uint8_t* out, int d, int h, int w,
                     mednet_stream stream);

/* ---- resampling between voxel grids (additive to ABI 3; the reference resamples nothing) ---------------------------------------------
 * Separable and table-driven: the host states an axis once (mednet_hip/resample.py: axis_table) and the kernels only execute it.
 * A table of an axis with n_out outputs is start int32[n_out], count int32[n_out], weight fp32[n_out][taps] (all 4-byte aligned):
 * output i reads the source indices start[i] .. start[i] + count[i] - 1 with the weights weight[i * taps + k]; slots at and above
 * count[i] are not read.  THE ARITHMETIC, pinned (fp32 throughout; tests/resample_util.py restates it).  A chain over the values
 * v[k] of a row (f16 and u8 widened first) is
 *   acc = w[0] * v[0];   acc = fmaf(w[k], v[k], acc)  for k = 1 .. count - 1,        in exactly this order.
 * A voxel outside a row's count never reaches the output (a NaN next to the support does not leak).  Inside the kernels count is
 * clamped to 1 .. taps and every index to the extent: any table is safe for memory.  No atomics, one owning thread per output
 * voxel: the same inputs give the same bits.
 * Refused before anything is launched, by both entries: a null pointer, an extent outside 1 .. 2048 or d * h * w >= 2^31 (a linear
 * voxel index fits 32 bits; channel offsets are held in size_t), on the way in or out, an axis outside 0 .. 2, c < 1, taps outside
 * 1 .. 64, ncls outside 1 .. 256, a table (or out_max) that is not 4-byte aligned (all MEDNET_E_SHAPE); an unknown dtype
 * (MEDNET_E_DTYPE).
 *
 * mednet_resample_axis: one pass.  src is c x d x h x w, dst the same with extent `axis` (0, 1, 2 counting within d x h x w)
 * replaced by n_out.  src_dtype and dst_dtype each MEDNET_F32, MEDNET_F16 or MEDNET_U8.  Stores: f32 as is, f16 one
 * round-to-nearest-even, u8 fminf(fmaxf(acc, 0), 255) and one rintf (nearest-even). */
int mednet_resample_axis(const void* src, int src_dtype, void* dst, int dst_dtype, int c, int d, int h, int w, int axis, int n_out,
                         const int* start, const int* count, const float* weight, int taps, mednet_stream stream);
/* mednet_resample_argmax: the fused way back -- one pass over the od x oh x ow output, no class volume at the output size.
 *   src     MEDNET_F32 / MEDNET_F16: ncls planes d x h x w of scores (probabilities, logits, anything);
 *           MEDNET_U8: ONE label volume d x h x w whose class-c score at a voxel is label == c ? 1 : 0 (one-hot linear resampling
 *           of a segmentation without the one-hot tensor; a label >= ncls scores for nobody)
 *   score   of (output voxel, class): the tensor product of the three tables (0: z, 1: y, 2: x) in the association of three axis
 *           passes run x, then y, then z with fp32 between them -- the x chain for every (z-tap, y-tap), then the y chain over
 *           those, then the z chain: bit for bit what mednet_resample_axis gives on axis 2, 1, 0 with fp32 destinations
 *   out     uint8 od x oh x ow (any address): the first maximum over the classes, the lowest class on ties (torch.argmax); a NaN
 *           score never wins against class 0
 *   out_max fp32 od x oh x ow or NULL: the winning score */
int mednet_resample_argmax(const void* src, int src_dtype, int ncls, int d, int h, int w, uint8_t* out, float* out_max, int od, int oh,
                           int ow, const int* start0, const int* count0, const float* weight0, int taps0, const int* start1,
                           const int* count1, const float* weight1, int taps1, const int* start2, const int* count2,
                           const float* weight2, int taps2, mednet_stream stream);

/* ---- intensity normalisation (additive to ABI 3; the reference normalises on the host) -------------------------------------------------
 * Sources are c x d x h x w, dense, MEDNET_F32, MEDNET_F16, MEDNET_I16 or MEDNET_U8; every value is converted to fp32 first (exact
 * for all four).  MEMBERSHIP: voxel (z, y, x) of channel c takes part iff mask[z, y, x] != 0 (mask: uint8 d x h x w at any address,
 * shared by the channels, NULL: every voxel) and its value is not NaN; n_nan counts a channel's NaN voxels inside the mask; +-inf
 * are values like any other.
 * Refused before anything is launched: a null pointer, an extent outside 1 .. 2048, d * h * w >= 2^31, channels < 1, ranks outside
 * 1 .. MEDNET_INTENSITY_MAX_RANKS, a level, pass or scheme that does not exist, a percentile outside 0 .. 100, a misaligned table,
 * workspace or source (all MEDNET_E_SHAPE); an unsupported dtype (MEDNET_E_DTYPE); a workspace smaller than the _ws_bytes query
 * answers (MEDNET_E_WORKSPACE).
 * THE ARITHMETIC, pinned (tests/intensity_util.py restates it):
 *   select      key(x): u = bits(x), x == 0 -> u = 0; key = u < 2^31 ? u | 2^31 : ~u.  Three levels of 11, 11, 10 key bits; integer
 *               histograms only (LDS integer atomics, 64-bit global integer adds): the value with rank r among the members, bit-equal
 *               to sort(members)[r]; a rank outside [0, n) gives NaN.
 *   moments     pass A: n, n_nan, min, max, sum x in fp64 (per thread, block tree, partial rows in fixed order), mean = sum / n;
 *               pass B: sum of d * d with d = x - mean, unfused; std = sqrt(sum / n) (population form).  n = 0: NaN.
 *   percentile  q of n: pos = q / 100 * (n - 1); ranks floor(pos), min(floor(pos) + 1, n - 1); t = pos - floor(pos);
 *               value = t == 0 ? a : a + (b - a) * t in fp64, each operation rounded on its own.
 *   table       float[c][4] = (lo, hi, sub, mul), computed in fp64 and rounded to fp32 once:
 *               zscore (-inf, +inf, mean, 1 / max(std, eps)); ct (p0, p1, mean, 1 / max(std, eps));
 *               rescale (p0, p1, p0, 1 / max(p1 - p0, eps)), p0 / p1 the first two percentiles.
 *   apply       y = (min(max(x, lo), hi) - sub) * mul in fp32, each operation rounded on its own; f16: one round-to-nearest-even
 *               store; outside the mask and at a NaN: fill.
 * The statistics table is c rows of MEDNET_INTENSITY_TABLE_BYTES: int64 n, int64 n_nan, fp32 min, fp32 max, fp64 mean, fp64 std.
 *
 * The accumulate form (select and moments): a level / pass is run over several volumes -- the cases of a data set -- before the
 * next one; MEDNET_INTENSITY_FIRST on the first volume of a level clears its counters, MEDNET_INTENSITY_LAST on the last one closes it
 * (select: the walk that refines every rank; moments: mean after pass 0, the table after either pass, std after pass 1).  The
 * workspace carries the state between the calls: the largest of the volumes' queries, untouched in between.  level / pass
 * MEDNET_INTENSITY_ALL: everything for one volume in one call (flags ignored).  Ranks then refer to the union of the members. */
enum { MEDNET_INTENSITY_MAX_RANKS = 8, MEDNET_INTENSITY_TABLE_BYTES = 40 };
enum { MEDNET_INTENSITY_ALL = -1, MEDNET_INTENSITY_FIRST = 1, MEDNET_INTENSITY_LAST = 2 };
enum { MEDNET_INTENSITY_ZSCORE = 0, MEDNET_INTENSITY_CT = 1, MEDNET_INTENSITY_RESCALE = 2, MEDNET_INTENSITY_PERCENTILES = 3 };
size_t mednet_intensity_select_ws_bytes(int channels, int nranks);
/* ranks: int64 [c][nranks] in device memory, zero-based; out: fp32 [c][nranks]; counts: int64 [c][2] = (n, n_nan) or NULL, written
 * when level 0 closes; level 0 .. 2 or MEDNET_INTENSITY_ALL. */
int mednet_intensity_select(const void* src, int dtype, const uint8_t* mask, int c, int d, int h, int w, const int64_t* ranks,
                            int nranks, float* out, int64_t* counts, int level, int flags, void* ws, size_t ws_bytes,
                            mednet_stream stream);
size_t mednet_intensity_moments_ws_bytes(int c, int d, int h, int w);
/* pass 0 (A), 1 (B) or MEDNET_INTENSITY_ALL; table: the statistics table (written when a pass closes). */
int mednet_intensity_moments(const void* src, int dtype, const uint8_t* mask, int c, int d, int h, int w, int pass, int flags,
                             void* table, void* ws, size_t ws_bytes, mednet_stream stream);
/* The ranks behind nq percentiles (q0 .. q3, the first nq count) of every channel's n in the statistics table: ranks int64
 * [c][2 nq] as select takes them, frac fp64 [c][nq] = t.  A tiny kernel: select needs no host round trip. */
int mednet_intensity_ranks(const void* table, int c, double q0, double q1, double q2, double q3, int nq, int64_t* ranks, double* frac,
                           mednet_stream stream);
/* One workgroup: statistics -> the apply table `out` of `scheme`, and / or the percentiles pct fp64 [c][nq] (NULL: not wanted;
 * MEDNET_INTENSITY_PERCENTILES: only these).  order: select's output for mednet_intensity_ranks' ranks, fp32 [c][2 nq]. */
int mednet_intensity_params(int scheme, const void* table, const float* order, const double* frac, int nq, int c, double eps,
                            double* pct, float* out, mednet_stream stream);
/* One pass, dst MEDNET_F32 or MEDNET_F16; table: float[c][4] in device memory; src == dst is legal for equal dtypes. */
int mednet_intensity_apply(const void* src, int src_dtype, void* dst, int dst_dtype, const uint8_t* mask, int c, int d, int h, int w,
                           const float* table, float fill, mednet_stream stream);
/* mask[z, y, x] = any_c(src[c, z, y, x] != 0) as 0 / 1 (NaN counts as non-zero); box: int32[6] = the inclusive (z0, y0, x0, z1, y1,
 * x1) of the mask by integer min / max; an all-zero volume gives (0, 0, 0, -1, -1, -1). */
int mednet_nonzero_mask(const void* src, int dtype, int c, int d, int h, int w, uint8_t* mask, int32_t* box, mednet_stream stream);

/* ---- image degradation of a training batch (additive to ABI 3; the reference degrades nothing) -------------------------------------------
 * Gaussian noise, Gaussian blur and simulated low resolution (mednet_hip/sampler.py: ImageDegradation).  Both entries work on
 * rows x spatial dense fp32, rows = B * C of the batch tensor; both refuse bad arguments before anything is launched; no atomics,
 * one owning thread per element: the same inputs give the same bits.
 *
 * mednet_noise_patches: in place, data[r][v] = fmaf(std[r], z(seed, r, v), data[r][v]).  std: fp32 [rows] in device memory (4-byte
 * aligned); a row with std[r] == 0 is neither read nor written.  z is a pure function of (seed, r, v) -- not of the grid, of other
 * rows' std or of the batch size.  THE ARITHMETIC, pinned (tests/degrade_util.py restates it):
 *   block j = v >> 2, lane v & 3;
 *   (r0, r1, r2, r3) = philox4x32-10(counter = (j, r, 0, 0), key = (seed & 0xffffffff, seed >> 32)) -- multipliers 0xD2511F53 and
 *   0xCD9E8D57, key increments 0x9E3779B9 and 0xBB67AE85, ten rounds;
 *   lanes 0 and 1 come from the pair (r0, r1), lanes 2 and 3 from (r2, r3); for a pair (a, b):
 *   u1 = ((a >> 8) + 1) * 2^-24 (in (0, 1]: the logarithm is finite), u2 = (b >> 8) * 2^-24, rad = sqrtf(-2 * logf(u1)),
 *   z_even = rad * cospif(2 * u2), z_odd = rad * sinpif(2 * u2).
 * One thread owns one block of four voxels: a 16-byte load and store where the address allows, scalar accesses otherwise (the
 * tail of a row when spatial % 4 != 0).
 * Refused (MEDNET_E_SHAPE): a null pointer, rows < 1, spatial < 1, spatial >= 2^32 (the counter's word 0 never wraps: "32-bit
 * index"), a std (or data) pointer that is not 4-byte aligned. */
int mednet_noise_patches(float* data, const float* std, uint64_t seed, int rows, size_t spatial, mednet_stream stream);
/* mednet_filter_rows: one extent-preserving axis pass over the whole batch, out of place (src != dst).  Every row is a d x h x w
 * volume; n is the extent of `axis` (0: d, 1: h, 2: w).
 *   row_table int32 [rows]: the table of row r, -1 .. n_tables - 1.  A row with -1 (or any entry outside that range) is COPIED bit
 *             for bit, NaN payloads and -0.0 included.
 *   count     int32 [n_tables][n], index int32 [n_tables][n][taps], weight fp32 [n_tables][n][taps] (all 4-byte aligned).
 * THE ARITHMETIC, pinned: output i of a row with table t is the chain over the row's values v along the axis
 *   acc = weight[(t n + i) taps] * v[index[(t n + i) taps]];
 *   acc = fmaf(weight[.. + k], v[index[.. + k]], acc)  for k = 1 .. count[t n + i] - 1,          in exactly this order,
 * fp32 throughout: the chain of mednet_resample_axis with an explicit index per tap in place of start + k.  Slots at and above
 * count are never read (a NaN next to the support does not leak).  Inside the kernels count is clamped to 1 .. taps and every index
 * to 0 .. n - 1 (csrc/degrade_index.h): any table is safe for memory.
 * Refused (MEDNET_E_SHAPE): a null pointer, an extent outside 1 .. 2048, d * h * w >= 2^31, axis outside 0 .. 2, rows < 1,
 * n_tables < 1, taps outside 1 .. 64, src == dst, a table (or volume) that is not 4-byte aligned. */
int mednet_filter_rows(const float* src, float* dst, int rows, int d, int h, int w, int axis, const int* row_table, int n_tables,
                       const int* count, const int* index, const float* weight, int taps, mednet_stream stream);

#ifdef __cplusplus
}
#endif
#endif
