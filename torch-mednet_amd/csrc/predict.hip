// Inference path: the data movement around the forward kernels at prediction time, on the device.
//   grid_gather      midasmednet/dataset.py:349-390 (grid_patch_generator): np.pad + overlapping patch extraction; with a mirror
//                    mask (grid_gather_mirror, for blend.hip's test-time mirroring) the patch comes out reversed on the flagged axes
//   predict_assemble examples/predict.py:88-95 (argmax of the class logits, heat maps clipped to uint8) fused with
//                    GridPatchSampler.add_processed_batch (dataset.py:446-474): crop the overlap, clip at the volume
//                    edge, write into the result volume -- one pass over the logits, nothing intermediate in HBM.
#include "volume.h"

namespace mednet {

// original index of padded index q (pad of `ov` in front), or -1 for a constant-mode zero
__device__ __forceinline__ int pad_src(int q, int ov, int n, int mode) {
  int i = q - ov;
  if (mode == MEDNET_PAD_CONSTANT) return (i >= 0 && i < n) ? i : -1;
  // numpy 'symmetric': ... 1 0 | 0 1 2 ... n-1 | n-1 n-2 ...  with period 2n
  const int period = 2 * n;
  i %= period;
  if (i < 0) i += period;
  return i < n ? i : period - 1 - i;
}

__global__ __launch_bounds__(256) void grid_gather_kernel(const float* __restrict__ vol, const int* __restrict__ pos,
                                                          float* __restrict__ out, int c, int d, int h, int w, int pd,
                                                          int ph, int pw, int ov0, int ov1, int ov2, int mode, int mirror) {
  const size_t per = (size_t)c * pd * ph * pw;
  const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= per) return;
  const int b = blockIdx.y;
  const auto [cc, z, y, x] = voxel_czyx(i, pd, ph, pw);
  // bit k of `mirror` reverses patch axis k: voxel (z, y, x) holds what the unmirrored patch holds at (pd - 1 - z, ..)
  const int mz = (mirror & 1) ? pd - 1 - z : z, my = (mirror & 2) ? ph - 1 - y : y, mx = (mirror & 4) ? pw - 1 - x : x;
  const int sz = pad_src(pos[b * 3] + mz, ov0, d, mode), sy = pad_src(pos[b * 3 + 1] + my, ov1, h, mode),
            sx = pad_src(pos[b * 3 + 2] + mx, ov2, w, mode);
  float v = 0.f;
  if (sz >= 0 && sy >= 0 && sx >= 0) v = vol[(((size_t)cc * d + sz) * h + sy) * w + sx];
  out[(size_t)b * per + i] = v;
}

// one thread per voxel of the cropped window of one patch: all output channels of that voxel
__global__ __launch_bounds__(256) void predict_assemble_kernel(const float* __restrict__ logits, const int* __restrict__ pos,
                                                               uint8_t* __restrict__ result, int nh, int ncls, int d, int h,
                                                               int w, int pd, int ph, int pw, int cs0, int cs1, int cs2,
                                                               int cz, int cy, int cx) {
  const size_t win = (size_t)cz * cy * cx;
  const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= win) return;
  const int b = blockIdx.y;
  const auto [z, y, x] = voxel_zyx(i, cy, cx);
  const int gz = pos[b * 3] + z, gy = pos[b * 3 + 1] + y, gx = pos[b * 3 + 2] + x;
  if (gz >= d || gy >= h || gx >= w) return;  // the part of the last patches that hangs over the volume
  // The windows of one launch can overlap: the grid step on axis 0 is pd - 2 o0, the window pd - o0 - o1 long, so with o0 > o1
  // neighbours share o0 - o1 planes.  add_processed_batch writes the items in order -- the LAST row covering a voxel wins.  Items
  // of a launch have no order, so a thread leaves its voxel to any later row whose window holds it (rows are three ints, batches
  // small, the loads uniform); across launches stream order gives the same rule.
  for (int j = b + 1; j < (int)gridDim.y; ++j) {
    const int qz = gz - pos[j * 3], qy = gy - pos[j * 3 + 1], qx = gx - pos[j * 3 + 2];
    if (qz >= 0 && qz < cz && qy >= 0 && qy < cy && qx >= 0 && qx < cx) return;
  }
  const size_t pvox = (size_t)pd * ph * pw;
  const float* src = logits + (size_t)b * (nh + ncls) * pvox + ((size_t)(z + cs0) * ph + (y + cs1)) * pw + (x + cs2);
  const size_t vox = (size_t)d * h * w, dst = ((size_t)gz * h + gy) * w + gx;
  for (int k = 0; k < nh; ++k) result[(size_t)k * vox + dst] = heat_to_u8(src[(size_t)k * pvox]);
  result[(size_t)nh * vox + dst] = (uint8_t)argmax_first(src + (size_t)nh * pvox, pvox, ncls);  // argmax(softmax(x)) == argmax(x)
}

// ---- training-patch crop: MedDataset.__getitem__'s `vol[:, i0:i1, j0:j1, k0:k1].astype(..)`
//      (dataset.py:313-331) from a device-resident volume straight into a slot / channel range of the batch tensors
template <typename TS, typename TD>
__global__ __launch_bounds__(256) void crop_patches_kernel(const TS* __restrict__ src, const int* __restrict__ pos,
                                                           const int* __restrict__ slot, TD* __restrict__ out, int c, int d,
                                                           int h, int w, int c_total, int c_off, int pd, int ph, int pw) {
  const size_t per = (size_t)c * pd * ph * pw;
  const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= per) return;
  const int b = blockIdx.y;
  const auto [cc, z, y, x] = voxel_czyx(i, pd, ph, pw);
  const TS v = src[(((size_t)cc * d + pos[b * 3] + z) * h + pos[b * 3 + 1] + y) * w + pos[b * 3 + 2] + x];
  out[(((size_t)slot[b] * c_total + c_off + cc) * pd + z) * ph * pw + (size_t)y * pw + x] = (TD)v;
}

}  // namespace mednet

using namespace mednet;

extern "C" int mednet_crop_patches(const void* src, int src_dtype, const int* pos, const int* slot, int count, void* out,
                                   int dst_dtype, int c, int d, int h, int w, int c_total, int c_off, int pd, int ph, int pw,
                                   mednet_stream stream) {
  MEDNET_REQUIRE(count > 0 && c > 0 && pd > 0 && ph > 0 && pw > 0 && pd <= d && ph <= h && pw <= w && c_off >= 0 &&
                     c_off + c <= c_total,
                 MEDNET_E_SHAPE, "crop_patches: bad shape (patch %dx%dx%d in %dx%dx%d, channels %d+%d of %d)", pd, ph, pw, d, h, w,
                 c_off, c, c_total);
  const dim3 grid(grid_blocks((size_t)c * pd * ph * pw, 256), count);
  hipStream_t s = (hipStream_t)stream;
#define CP_GO(TS_, TD_) hipLaunchKernelGGL((crop_patches_kernel<TS_, TD_>), grid, dim3(256), 0, s, (const TS_*)src, pos, slot, (TD_*)out, c, d, h, w, c_total, c_off, pd, ph, pw)
  if (src_dtype == MEDNET_F16 && dst_dtype == MEDNET_F32) CP_GO(_Float16, float);
  else if (src_dtype == MEDNET_F32 && dst_dtype == MEDNET_F32) CP_GO(float, float);
  else if (src_dtype == MEDNET_U8 && dst_dtype == MEDNET_U8) CP_GO(uint8_t, uint8_t);
  else return fail(MEDNET_E_DTYPE, "crop_patches: %d -> %d (supported: f16->f32, f32->f32, u8->u8)", src_dtype, dst_dtype);
#undef CP_GO
  return check_launch("crop_patches");
}

// both gather entries: `who` names the entry in the messages
static int grid_gather_go(const char* who, const float* volume, const int* pos, float* out, int batch, int c, int d, int h, int w,
                          int pd, int ph, int pw, int ov0, int ov1, int ov2, int pad_mode, int mirror, mednet_stream stream) {
  MEDNET_REQUIRE(batch > 0 && c > 0 && d > 0 && h > 0 && w > 0 && pd > 0 && ph > 0 && pw > 0, MEDNET_E_SHAPE, "%s: bad shape", who);
  MEDNET_REQUIRE(pad_mode == MEDNET_PAD_CONSTANT || pad_mode == MEDNET_PAD_SYMMETRIC, MEDNET_E_UNSUPPORTED,
                 "%s: pad mode %d (supported: constant, symmetric)", who, pad_mode);
  hipLaunchKernelGGL(grid_gather_kernel, dim3(grid_blocks((size_t)c * pd * ph * pw, 256), batch), dim3(256), 0, (hipStream_t)stream, volume,
                     pos, out, c, d, h, w, pd, ph, pw, ov0, ov1, ov2, pad_mode, mirror);
  return check_launch(who);
}

extern "C" int mednet_grid_gather(const float* volume, const int* pos, float* out, int batch, int c, int d, int h, int w,
                                  int pd, int ph, int pw, int ov0, int ov1, int ov2, int pad_mode, mednet_stream stream) {
  return grid_gather_go("grid_gather", volume, pos, out, batch, c, d, h, w, pd, ph, pw, ov0, ov1, ov2, pad_mode, 0, stream);
}

extern "C" int mednet_grid_gather_mirror(const float* volume, const int* pos, float* out, int batch, int c, int d, int h, int w,
                                         int pd, int ph, int pw, int ov0, int ov1, int ov2, int pad_mode, int mirror,
                                         mednet_stream stream) {
  MEDNET_REQUIRE(volume && pos && out, MEDNET_E_SHAPE, "grid_gather_mirror: null pointer");
  if (const int rc = mirror_check("grid_gather_mirror", mirror)) return rc;
  return grid_gather_go("grid_gather_mirror", volume, pos, out, batch, c, d, h, w, pd, ph, pw, ov0, ov1, ov2, pad_mode, mirror, stream);
}

extern "C" int mednet_predict_assemble(const float* logits, const int* pos, uint8_t* result, int batch, int num_heatmaps,
                                       int num_classes, int d, int h, int w, int pd, int ph, int pw, int crop_start0,
                                       int crop_start1, int crop_start2, int crop_d, int crop_h, int crop_w,
                                       mednet_stream stream) {
  MEDNET_REQUIRE(batch > 0 && num_heatmaps >= 0 && num_classes >= 1, MEDNET_E_SHAPE, "predict_assemble: bad channel counts");
  MEDNET_REQUIRE(crop_start0 >= 0 && crop_start1 >= 0 && crop_start2 >= 0 && crop_start0 + crop_d <= pd &&
                     crop_start1 + crop_h <= ph && crop_start2 + crop_w <= pw,
                 MEDNET_E_SHAPE, "predict_assemble: crop window outside the patch");
  const size_t win = (size_t)crop_d * crop_h * crop_w;
  if (win == 0) return MEDNET_OK;  // (the reference's slicing yields an empty window when an overlap is 0)
  hipLaunchKernelGGL(predict_assemble_kernel, dim3(grid_blocks(win, 256), batch), dim3(256), 0, (hipStream_t)stream,
                     logits, pos, result, num_heatmaps, num_classes, d, h, w, pd, ph, pw, crop_start0, crop_start1,
                     crop_start2, crop_d, crop_h, crop_w);
  return check_launch("predict_assemble");
}
