// Internal declarations shared by the convolution translation units.
#pragma once
#include <type_traits>

#include "common.h"

namespace mednet {

enum { MAP_CONV = 0, MAP_CT_FWD = 1, MAP_CT_DG = 2 };

struct ConvGeom {
  int n, od, oh, ow;  // output dims
  int id, ih, iw;     // input dims
  int k, m;           // input channels, output channels
  int ks;             // 3 or 1
  int in_planar, out_planar;
};

struct WgradGeom {
  int n, ad, ah, aw;  // dims of A's grid (the loop grid)
  int bd, bh, bw;     // dims of B's grid
  int ka, kb, ks, stride2;
  int a_planar, b_planar;
  size_t chunk;  // voxels per chunk (filled by the launcher)
};


template <int MAP>
int launch_direct(const void* x, const float* P, const float* bias, const void* skip, void* y, const ConvGeom& g,
                  int x_dtype, int y_dtype, hipStream_t s);
size_t wgrad_direct_ws_bytes(size_t nvox, int ka, int kb, int ks);
int launch_wgrad_direct(const void* A, const void* B, float* dw, WgradGeom g, int a_dtype, int b_dtype, void* ws,
                        size_t ws_bytes, hipStream_t s);
size_t channel_sum_ws_bytes(int n, size_t spatial, int c);
int launch_channel_sum(const void* x, float* out, int n, size_t spatial, int c, int planar, int dtype, void* ws,
                       size_t ws_bytes, hipStream_t s);
bool head_dgrad_supported(int cin, int cout, int ksize, int x_dtype, int x_layout, int y_layout);
int launch_head_dgrad(const void* dy, const float* Pb, void* dz, int n, size_t spatial, int m, int k, int out_dtype,
                      hipStream_t s);
int head_dgrad_gn_rows(size_t spatial, int k, int dtype);
int launch_head_dgrad_gn(const void* dy, const float* Pb, void* dz, const void* gy, const void* gz, int act, float* partial,
                         int n, size_t spatial, int m, int k, int dtype, hipStream_t s);
bool head_vox_supported(int k);
int launch_head_fwd_vox(const void* z, const float* Pb, const float* bias, float* y, int n, size_t spatial, int k, int m,
                        int z_dtype, hipStream_t s);
bool wgrad_1x1_supported(int cin, int cout, int ksize, int x_layout, int dy_layout, int dy_dtype);
size_t wgrad_1x1_ws_bytes(int n, size_t spatial, int cin, int cout);
int launch_wgrad_1x1(const void* z, const void* dy, float* dw, int n, size_t spatial, int cin, int cout, int z_dtype,
                     void* ws, size_t ws_bytes, hipStream_t s);
bool wgrad_c1_supported(int cin, int cout, int ksize, int x_layout, int dy_layout);
size_t wgrad_c1_ws_bytes(int n, int d, int h, int w, int cout);
bool wgrad_c1_gn_supported(int cout, int x_dtype, int dtype);
int launch_wgrad_c1_gn(const void* x, const void* dz, const void* y, const float* coef, const float* bcoef, int act, float* dw,
                       int n, int d, int h, int w, int cout, int x_dtype, int dtype, void* ws, size_t ws_bytes, hipStream_t s);
int launch_wgrad_c1(const void* x, const void* dy, float* dw, int n, int d, int h, int w, int cout, int x_dtype,
                    int dy_dtype, void* ws, size_t ws_bytes, hipStream_t s, bool split_bf16 = false);
// multi-channel first layer (Cin = 2, 3, 4): the matrix-core weight gradient of conv_first_mfma.inc, plain and GroupNorm form
bool wgrad_cm_supported(int cin, int cout, int ksize, int x_dtype, int dy_dtype, int dy_layout);
bool wgrad_cm_gn_supported(int cin, int cout, int x_dtype, int dtype);
size_t wgrad_cm_ws_bytes(int n, int d, int h, int w, int cin, int cout);
int wgrad_cm_plan(int n, int d, int h, int w, int cin, int cout, int dtype, bool gn, int* out4);
int launch_wgrad_cm(const void* x, int x_layout, const void* dz, const void* y, const float* coef, const float* bcoef, int act,
                    float* dw, int n, int d, int h, int w, int cin, int cout, int dtype, void* ws, size_t ws_bytes, hipStream_t s);
int launch_pack_f32(const float* w, float* Pf, float* Pb, int cin, int cout, int T, int transposed_src, hipStream_t s);

// loss.hip: the single-workgroup fp64 combines of the per-workgroup loss partials
int launch_hm_finalize(const float* partial, const float* cweight, float* loss, int n, int c, int nblocks, size_t spatial,
                       hipStream_t s);
int launch_dice_finalize(const float* partial, const float* weight, float* loss, float* saved, int c, int nblocks, float eps,
                         hipStream_t s, float* dice_out = nullptr);
// partial[nblocks][2] = {sum w_y nll, sum w_y} -> *loss = num / den, saved[0] = den (ce_finalize_kernel)
int launch_ce_finalize(const float* partial, float* loss, float* saved, int nblocks, hipStream_t s);
// Dice rows + CE rows -> *loss = fl(dice + ce), saved = [c][2] {I, D} then sum w_y (dice_ce_finalize_kernel)
int launch_dice_ce_finalize(const float* partial, const float* partial_ce, const float* weight, float* loss, float* saved, int c,
                            int nblocks, float eps, hipStream_t s, float* dice_out = nullptr);
// the one of the three that class loss `kind` (MEDNET_CLASS_*) takes; a fused head's rows: [rows][c][2] (Dice), [rows][2] (CE)
int launch_class_finalize(int kind, const float* dice_partial, const float* ce_partial, const float* weight, float* loss, float* saved,
                          int c, int rows, float eps, hipStream_t s);
// one workspace for both: all the Dice rows first, then all the CE rows (a CE head has its rows at the front)
inline int launch_class_finalize(int kind, const float* partial, const float* weight, float* loss, float* saved, int c, int rows,
                                 float eps, hipStream_t s) {
  const float* ce_partial = kind == MEDNET_CLASS_DICE_CE ? partial + (size_t)rows * c * 2 : partial;
  return launch_class_finalize(kind, partial, ce_partial, weight, loss, saved, c, rows, eps, s);
}

// The fused class heads' launches: the run-time class loss `ce` (MEDNET_CLASS_*) as the compile-time KIND of a kernel instantiation,
// f(std::integral_constant<int, KIND>), and the launch's name for check_launch, STEM + {"", "_ce", "_dice_ce"} + DIR
template <class F>
inline void for_class_kind(int ce, F&& f) {
  if (ce == MEDNET_CLASS_DICE_CE) f(std::integral_constant<int, MEDNET_CLASS_DICE_CE>{});
  else if (ce) f(std::integral_constant<int, MEDNET_CLASS_CE>{});
  else f(std::integral_constant<int, MEDNET_CLASS_DICE>{});
}
#define MEDNET_CLASS_KIND_NAME(ce, STEM, DIR) ((ce) == MEDNET_CLASS_DICE_CE ? STEM "_dice_ce" DIR : (ce) ? STEM "_ce" DIR : STEM DIR)

// 16-bit matrix-core kernels, conv_mfma.hip (namespace mednet: bf16; api.hip declares the same set in namespace mednet_f16
// for the fp16 build of that file)
#include "conv_mfma_decl.inc"
// the fp32 weights W[co][ci] of a 1x1x1 head inside its packed buffer: the backward section of its one tap, Pb[0][co][ci]
inline const float* head_weights_f32(const void* packed, int cin, int cout) {
  return (const float*)((const char*)packed + pack_layout(cin, cout, 1).f32_bwd);
}

// fp32 matrix-core kernels (v_mfma_f32_32x32x2_f32), conv_f32_mfma.hip: the parity mode's 3x3x3 family
bool conv_f32_mfma_enabled();
int launch_conv_f32_mfma(const void* x, const float* P, const float* bias, void* y, int n, int d, int h, int w, int k, int m,
                         hipStream_t s);
int launch_convt_dgrad_f32_mfma(const void* dy, const float* Pb, void* dx, int n, int d, int h, int w, int cin, int cout,
                                hipStream_t s);
int launch_convt_fwd_f32_mfma(const void* x, const float* Pf, const float* bias, const void* skip, void* y, int n, int d, int h,
                              int w, int cin, int cout, hipStream_t s);
size_t wgrad_f32_mfma_ws_bytes(int n, int d, int h, int w, int ka, int kb, int stride2);
int launch_wgrad_f32_mfma(const void* x, const void* dy, float* dw, int n, int d, int h, int w, int cin, int cout, void* ws,
                          size_t ws_bytes, hipStream_t s);
int launch_convt_wgrad_f32_mfma(const void* x, const void* dy, float* dw, int n, int d, int h, int w, int cin, int cout, void* ws,
                                size_t ws_bytes, hipStream_t s);

// split-bf16 matrix-core kernels (three v_mfma_f32_32x32x16_bf16 per product on hi/lo halves), conv_x3_mfma.hip: the parity
// mode's 3x3x3 family at bf16 matrix-core speed.  `sec_hi` = the layer's bf16 fragment image (PackLayout::mfma_fwd / mfma_bwd),
// the low image sits PackLayout::lo_delta bytes behind it (mednet_conv3d_pack_elt(MEDNET_F32)).
bool conv_x3_enabled();
bool conv_x3_supported(int cin, int cout, int ksize);
bool conv_x3_fits(int d, int h, int w, int c);
int conv_x3_stats_rows(int n, int d, int h, int w, int cout);
int launch_conv_x3(const void* x, const void* sec_hi, size_t lo_delta, const float* bias, void* y, int n, int d, int h, int w, int k,
                   int m, float* stats, hipStream_t s);
bool conv_c1_x3_supported(int cin, int cout, int ksize);
int conv_c1_x3_stats_rows(int d, int h, int w);
int launch_conv_c1_x3(const void* x, const float* w_pf, const float* bias, void* y, int n, int d, int h, int w, int cout,
                      float* stats, hipStream_t s);
int launch_conv_x3_dgrad(const void* dy, const void* sec_hi, size_t lo_delta, void* dx, int n, int d, int h, int w, int k, int m,
                         const void* add, const void* gn_y, const float* gn_coef, int gn_act, float* gn_partial, hipStream_t s);
int launch_convt_dgrad_x3(const void* dy, const void* sec_hi, size_t lo_delta, void* dx, int n, int d, int h, int w, int cin,
                          int cout, hipStream_t s);
int launch_convt_fwd_x3(const void* x, const void* sec_hi, size_t lo_delta, const float* bias, const void* skip, void* y, int n,
                        int d, int h, int w, int cin, int cout, hipStream_t s);
size_t wgrad_x3_ws_bytes(int n, int d, int h, int w, int cin, int cout, int workgroups);
bool wgrad_c1_x3_supported(int cout, int x_dtype, int dy_dtype);
int wgrad_c1_x3_blocks(int n, int d, int h, int w);
int launch_wgrad_c1_x3(const void* x, const void* dy, float* part, int n, int d, int h, int w, hipStream_t s);
int launch_wgrad_x3(const void* x, const void* dy, float* dw, int n, int d, int h, int w, int cin, int cout, void* ws,
                    size_t ws_bytes, hipStream_t s, int workgroups);

size_t convt_wgrad_x3_ws_bytes(int n, int d, int h, int w, int cin, int cout, int workgroups);
int launch_convt_wgrad_x3(const void* x, const void* dy, float* dw, int n, int d, int h, int w, int cin, int cout, void* ws,
                          size_t ws_bytes, hipStream_t s, int workgroups);

}  // namespace mednet
