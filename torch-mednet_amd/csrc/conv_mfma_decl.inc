// Declarations of what conv_mfma.hip defines (included inside namespace mednet by conv.h, and once more inside namespace
// mednet_f16 by api.hip: the fp16 build of that file).  No include guard on purpose.
// Byte offsets of the sections of a packed weight buffer (mednet_conv3d_pack); identical for bf16 and fp16 (2-byte elements).
struct PackLayout {
  int taps;
  size_t f32_fwd, f32_bwd;    // float [T][Cin][Cout], float [T][Cout][Cin] (taps mirrored for Conv3d sources)
  size_t mfma_fwd, mfma_bwd;  // 16-bit fragment-ordered images for the MFMA kernels (0 bytes when not applicable)
  size_t mfma_bytes;          // size of ONE mfma section
  size_t lo_delta;            // the LOW images of the split-bf16 contraction sit this many bytes behind mfma_fwd / mfma_bwd
  size_t total;
};
PackLayout pack_layout(int cin, int cout, int ksize);
// one layer of mednet_conv3d_pack_many, as the batched kernel reads it (64 bytes; built by mednet_conv3d_pack_table)
struct PackJobDev {
  const float* w;
  void* sec_fwd;
  void* sec_bwd;
  float* Pf;
  float* Pb;
  int cin, cout, transposed;
  unsigned nblocks;
  int lo_delta;  // PackLayout::lo_delta (the low images are written only by a launch that asks for them)
  unsigned first_block;  // blocks of the layers before this one (the launch is ONE dense range of blocks over all layers)
};
bool conv_mfma_fits(int n, int d, int h, int w, int c);
bool conv_mfma_supported(int cin, int cout, int ksize, int x_dtype, int y_dtype, int x_layout, int y_layout, bool bias);
int launch_conv_mfma(const void* x, const void* packed_section, void* y, int n, int d, int h, int w, int cin, int cout,
                     int x_dtype, int y_dtype, float* gn_partial, hipStream_t s, int act = MEDNET_ACT_NONE,
                     const void* add = nullptr, size_t lo_delta = 0);  // lo_delta != 0: split weights, the low image that far behind
int launch_conv_mfma_gnb(const void* dy, const void* packed_section, void* dx, int n, int d, int h, int w, int cin, int cout,
                         const void* add, const void* gn_y, const float* gn_coef, int gn_act, float* gn_partial, hipStream_t s,
                         size_t lo_delta = 0);
int conv_mfma_plan(int n, int d, int h, int w, int cin, int cout, bool gnb, int stride, int* out, bool split = false);
int conv_mfma_stats_chunks(int n, int d, int h, int w, int cin, int cout, bool gnb = false, bool split = false);  // gnb: rows of the data-gradient form
int launch_pack_mfma(const float* w, void* sec_fwd, void* sec_bwd, float* Pf, float* Pb, int cin, int cout, int T,
                     int transposed_src, hipStream_t s, size_t lo_delta = 0);
unsigned pack_mfma_blocks(int cin, int cout);
int launch_pack_mfma_many(const void* table_device, int njobs, unsigned max_blocks, hipStream_t s, int with_low = 0);
bool wgrad_mfma_supported(int cin, int cout, int ksize, int x_dtype, int dy_dtype, int x_layout, int dy_layout);
bool wgrad_mfma_fits(int n, int d, int h, int w, int cmax, int scale);
bool wgrad_mfma_coresident(int d, int h, int w);
int wgrad_mfma_plan(int n, int d, int h, int w, int cin, int cout, int workgroups, int* out);
size_t wgrad_mfma_ws_bytes(int n, int d, int h, int w, int cin, int cout, int ksize, int workgroups);
int launch_wgrad_mfma(const void* x, const void* dy, float* dw, int n, int d, int h, int w, int cin, int cout, int dtype,
                      void* ws, size_t ws_bytes, hipStream_t s, int workgroups);
int launch_convt_fwd_mfma(const void* x, const void* sec, const float* bias, const void* skip, void* y, int n, int d,
                          int h, int w, int cin, int cout, hipStream_t s, size_t lo_delta = 0);
int launch_convt_dgrad_mfma(const void* dy, const void* packed_section, void* dx, int n, int d, int h, int w, int cin,
                            int cout, hipStream_t s, size_t lo_delta = 0);
int convt_dgrad_gn_rows(int n, int d, int h, int w, int cin, int cout, bool split = false);
int launch_convt_dgrad_gn_mfma(const void* dy, const void* packed_section, void* dx, const void* gn_y, const void* gn_z, int gn_act,
                               float* gn_partial, int n, int d, int h, int w, int cin, int cout, hipStream_t s, size_t lo_delta = 0);
size_t convt_wgrad_mfma_ws_bytes(int n, int d, int h, int w, int cin, int cout, int workgroups);
int launch_convt_wgrad_mfma(const void* x, const void* dy, float* dw, int n, int d, int h, int w, int cin, int cout,
                            void* ws, size_t ws_bytes, hipStream_t s, int workgroups);

// conv_first_mfma.inc: the first layer (Cin = 1 .. 4; x fp32, planar or channels-last by `x_layout`, or with one channel in the
// storage type)
bool conv_first_mfma_supported(int cin, int cout, int ksize, int x_dtype, int y_dtype, int y_layout, bool bias);
int conv_first_stats_chunks(int n, int d, int h, int w, int cout);
int launch_conv_first_mfma(const void* x, int x_layout, int x_dtype, const float* w_pf, void* y, int n, int d, int h, int w, int cin,
                           int cout, float* gn_partial, hipStream_t s, int split = 0);
bool wgrad_first_mfma_supported(int cin, int cout, int x_dtype, int dy_dtype);
void wgrad_first_mfma_plan(int n, int d, int h, int w, int cin, int cout, bool gn, int* out4);  // {workgroups, NB, workgroups per CU, LDS bytes}
int wgrad_first_mfma_blocks(int n, int d, int h, int w, int cin, int cout, bool gn);  // (the plain form never has fewer)
// gn_y != NULL: `dy` is dz and GroupNorm's backward (coefficient tables [n][cout][2] and [n][cout][3]) is applied on the way in
int launch_wgrad_first_mfma(const void* x, int x_layout, int x_dtype, const void* dy, float* part, int n, int d, int h, int w, int cin,
                            int cout, hipStream_t s, const void* gn_y = nullptr, const float* gn_coef = nullptr,
                            const float* gn_bcoef = nullptr, int gn_act = 0);

// head_mfma.hip: the landmark head (1x1x1 conv 32 -> nh heat maps + ncls classes) fused with its two losses, matrix-core form
bool head_lm_supported(int cin, int nh, int ncls, int dtype, size_t spatial);
int head_lm_chunks(size_t spatial);  // workgroups per sample = rows per sample of every partial
size_t head_lm_ws_bytes(int n, size_t spatial, int nh, int ncls);
// ce = 0: the class term is DiceLoss.  ce = 1: nn.CrossEntropyLoss(cls_weight, ignore) (softmax; `sigmoid` and `eps` are not read):
// ce_partial [n][chunk][2] for ce_finalize, and dice_partial takes dice_metric's unweighted, unmasked sums; the backward reads
// saved[0] = sum w_y of that forward.  ce = 2: Dice + cross-entropy (softmax, no ignore_index); the forward runs the ce = 1 form, whose
// rows hold both terms' sums, the backward reads saved = [ncls][2] {I, D}, then sum w_y.
int launch_head_lm_fwd(const void* z, const float* W, const float* bias, const void* tgt, int64_t tgt_sn, const void* lab,
                       int64_t lab_sn, const float* cls_weight, float* logits, float* hm_partial, float* dice_partial, float* ce_partial,
                       int n, size_t spatial, int nh, int ncls, int kind, int ce, int sigmoid, int ignore, hipStream_t s);
int launch_head_lm_bwd(const void* z, const float* W, const float* bias, const void* tgt, int64_t tgt_sn, const void* lab,
                       int64_t lab_sn, const float* saved, const float* cls_weight, const float* reg_weight, const float* dcls,
                       const float* dreg, float eps, void* dz, const void* gn_y, int gn_act, float* gn_partial, float* dw, float* db,
                       int n, size_t spatial, int nh, int ncls, int kind, int ce, int sigmoid, int ignore, void* ws, size_t ws_bytes,
                       hipStream_t s);

// head_mfma.hip: the segmentation head (1x1x1 conv 32 -> 5 .. 16 classes) fused with DiceLoss (ce = 0) or nn.CrossEntropyLoss
// (ce = 1, softmax), matrix-core form.  `partial`: [n][chunk][ncls][2] for dice_finalize (ce = 0), [n][chunk][2] for ce_finalize
// (ce = 1), the first followed by the second for their sum (ce = 2: softmax, no ignore_index; saved = [ncls][2], then sum w_y);
// chunks = head_lm_chunks(spatial).  Labels uint8, base and sample stride multiples of 4 bytes.
bool head_seg_supported(int cin, int ncls, int dtype, size_t spatial);
size_t head_seg_ws_bytes(int n, size_t spatial, int ncls);
int launch_head_seg_fwd(const void* z, const float* W, const float* bias, const void* lab, int64_t lab_sn, const float* cls_weight,
                        float* logits, float* partial, int n, size_t spatial, int ncls, int ce, int sigmoid, int ignore, hipStream_t s);
int launch_head_seg_bwd(const void* z, const float* W, const float* bias, const void* lab, int64_t lab_sn, const float* saved,
                        const float* cls_weight, const float* dloss, float eps, void* dz, const void* gn_y, int gn_act,
                        float* gn_partial, float* dw, float* db, int n, size_t spatial, int ncls, int ce, int sigmoid, int ignore,
                        void* ws, size_t ws_bytes, hipStream_t s);

// ds_head.hip: the auxiliary head of a coarser decoder level (cin = 64 .. 256 in steps of 32 -> 1 .. 16 classes) fused with its class
// loss against the full-resolution uint8 labels (extents . x H x Wf) read at stride 2^shift; level extents d x h x w.  `partial` and `ce`
// as launch_head_seg_fwd's; the backward adds `d_pass` (nullable) in fp32 before the one rounding of dz.
bool ds_head_supported(int cin, int ncls, int dtype, size_t spatial);
int ds_head_chunks(size_t spatial);  // workgroups per sample = rows per sample of every partial
size_t ds_head_ws_bytes(int n, size_t spatial, int cin, int ncls);
int launch_ds_head_fwd(const void* z, const float* W, const float* bias, const void* lab, int64_t lab_sn, const float* cls_weight,
                       float* partial, int n, int d, int h, int w, int H, int Wf, int shift, int cin, int ncls, int ce, int sigmoid,
                       int ignore, hipStream_t s);
int launch_ds_head_bwd(const void* z, const float* W, const float* bias, const void* lab, int64_t lab_sn, const float* saved,
                       const float* cls_weight, const float* dloss, float eps, const void* d_pass, void* dz, float* dw, float* db, int n,
                       int d, int h, int w, int H, int Wf, int shift, int cin, int ncls, int ce, int sigmoid, int ignore, void* ws,
                       size_t ws_bytes, hipStream_t s);
