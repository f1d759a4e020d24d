// GPU crop / pad / resize / normalise of LineMOD frames -- the per-sample body of
// LineMODDatasetRGBD.__getitem__ (data/dataset_rgbd.py:104-206) and
// LineMODDatasetRGB.__getitem__ (data/dataset_rgb.py:95-145) after the file reads,
// batched: one launch turns B full frames (640x480 RGB u8 + u16 depth in mm) into
// the model inputs the DataLoader would have produced.
//
// One thread per output pixel (all three colour channels + depth): square crop
// geometry recomputed per thread from the sample's jittered bbox (a few scalar
// double ops, exactly the reference's Python arithmetic), zero padding folded into
// the gather (pixels outside the frame read as 0 = cv2.copyMakeBorder constant 0),
// cv2.resize INTER_LINEAR restated (8U: 11-bit fixed-point weights, vertical pass
// as OpenCV's SIMD body rounds; 16U: float weights, round-half-even; exact 2x:
// INTER_AREA), then ToTensor/Normalize and the depth normalisation.  Outputs are
// NCHW fp32 (rgb), (B,1,S,S) / (B,S,S) fp32 (depth), written coalesced along x.
// Built with -ffp-contract=off: every fp32 op rounds like numpy / torch-CPU.
// HBM-bound gather; algorithmic bytes per crop: <= 5 * crop^2 read (clipped to
// the frame) + S^2 * (12 + 4 + 4) written.
//
// The *_indexed entry points draw the same crops from a device-resident frame store:
// a device vector of sample indices picks table rows (frame, bbox, K, labels) and
// through them the frames; the per-pixel body is shared (crop_pixel).
//
// pose6d_crop_detections is the inference scripts' flavour of the same crop
// (scripts/inference/inference_rgbd_geometric.py:110-182): N detector boxes (x1, y1, x2, y2)
// over F frames, depth resized as float32, centre and intrinsics in double with one cast.
#include <math.h>

#include "common.h"

namespace {

constexpr int kThreads = 256;
constexpr int kCoefBits = 11;
constexpr int kCoefScale = 1 << kCoefBits;

struct CropGeom {
  int x1, y1;      // crop origin in ORIGINAL image coordinates (may be negative)
  int n;           // crop side int(size)
  int pad_l, pad_t;
  int x1p, y1p;    // origin in padded coordinates (dataset_rgbd.py:138-139)
};

// dataset_rgbd.py:120-139 (Python float = double, int() truncates toward zero)
__device__ __forceinline__ CropGeom crop_geom(const int32_t* bb, int H, int W) {
  const int x = bb[0], y = bb[1], w = bb[2], h = bb[3];
  const double c_x = (double)x + (double)w / 2.0, c_y = (double)y + (double)h / 2.0;
  const double size = (double)(w > h ? w : h) * 1.2;
  CropGeom g;
  g.x1 = (int)(c_x - size / 2.0);
  g.y1 = (int)(c_y - size / 2.0);
  g.n = (int)size;
  if (g.n < 1) g.n = 1;   // the reference raises on an empty crop (cv2.resize)
  g.pad_l = g.x1 < 0 ? -g.x1 : 0;
  g.pad_t = g.y1 < 0 ? -g.y1 : 0;
  const int pad_r = g.x1 + g.n - W > 0 ? g.x1 + g.n - W : 0;
  const int pad_b = g.y1 + g.n - H > 0 ? g.y1 + g.n - H : 0;
  const bool padded = g.pad_l > 0 || g.pad_t > 0 || pad_r > 0 || pad_b > 0;
  g.x1p = padded ? g.x1 + g.pad_l : g.x1;
  g.y1p = padded ? g.y1 + g.pad_t : g.y1;
  return g;
}

// cv::resizeGeneric_ tables for one output index: fx = (float)((d + 0.5) * scale - 0.5),
// sx = floor(fx), fx -= sx; x only: reset to (0, 0) / (n-1, 0) at the edges
__device__ __forceinline__ void lin_coef(int d, int n, int S, bool clamp_edges, int& s, float& f) {
  const double scale = 1.0 / ((double)S / (double)n);
  f = (float)(((double)d + 0.5) * scale - 0.5);
  s = (int)floorf(f);
  f = f - (float)s;
  if (clamp_edges) {
    if (s < 0) { f = 0.f; s = 0; }
    if (s >= n - 1) { f = 0.f; s = n - 1; }
  }
}

__device__ __forceinline__ int fix_coef(float c) { return (int)rintf(c * (float)kCoefScale); }   // cvRound

// One output pixel of crop b (and, on its pix == 0 thread, the crop's centre and
// intrinsics).  img / dimg: the sample's frame; ba / bo / k: the sample's jittered bbox,
// original bbox and K rows.  Outputs are indexed by b.  Shared by the contiguous-batch
// kernel and the frame-store (indexed) kernel, so the two cannot drift apart.
// kFloatDepth (compile time; false keeps the dataset flavour's code as it was): the
// inference scripts' depth, resized as float32 (cv2.resize(crop_depth.astype(np.float32)),
// inference_rgbd_geometric.py:142) -- the 16U branch's coefficients and mul + add without
// the rounding to whole millimetres and the saturation; exact 2x: (a + b + c + d) * 0.25f,
// exact for uint16 inputs in any order.
template <bool kFloatDepth>
__device__ __forceinline__ void crop_pixel(
    int b, int pix, const uint8_t* __restrict__ img, int bgr, const uint16_t* __restrict__ dimg, int H, int W,
    const int32_t* __restrict__ bo, const int32_t* __restrict__ ba, const float* __restrict__ k, int S,
    const float* __restrict__ mean_std, float* __restrict__ rgb_out, float* __restrict__ depth_out,
    float* __restrict__ depth_raw_out, float* __restrict__ center_out, float* __restrict__ K_out,
    uint8_t* __restrict__ u8_out) {
  const CropGeom g = crop_geom(ba, H, W);
  const float scale32 = (float)((double)S / (double)g.n);   // np.float32(img_size / crop_size)

  if (pix == 0) {
    if (center_out) {
      // dataset_rgbd.py:105,148-156 (float32 arithmetic, NEP 50 weak Python scalars)
      const float cgx = (float)((double)bo[0] + (double)bo[2] / 2.0);
      const float cgy = (float)((double)bo[1] + (double)bo[3] / 2.0);
      float ccx = (cgx + (float)g.pad_l) - (float)g.x1p;
      float ccy = (cgy + (float)g.pad_t) - (float)g.y1p;
      ccx = fminf(fmaxf(ccx * scale32, 0.f), (float)(S - 1));
      ccy = fminf(fmaxf(ccy * scale32, 0.f), (float)(S - 1));
      center_out[2 * b] = ccx;
      center_out[2 * b + 1] = ccy;
    }
    if (K_out) {
      // dataset_rgbd.py:159-169
      float* ko = K_out + 9 * b;
      ko[0] = k[0] * scale32; ko[1] = 0.f; ko[2] = ((k[2] + (float)g.pad_l) - (float)g.x1p) * scale32;
      ko[3] = 0.f; ko[4] = k[4] * scale32; ko[5] = ((k[5] + (float)g.pad_t) - (float)g.y1p) * scale32;
      ko[6] = 0.f; ko[7] = 0.f; ko[8] = 1.f;
    }
  }
  if (pix >= S * S) return;
  const int oy = pix / S, ox = pix - oy * S;
  const int n = g.n;

  // crop pixel (r, c) -> frame pixel (y1 + r, x1 + c); zero outside the frame
  auto in_frame = [&](int r, int c, int64_t& off) {
    const int yy = g.y1 + r, xx = g.x1 + c;
    off = (int64_t)yy * W + xx;
    return (unsigned)yy < (unsigned)H && (unsigned)xx < (unsigned)W;
  };
  auto px3 = [&](int r, int c, int (&v)[3]) {
    int64_t off;
    if (in_frame(r, c, off)) {
      const uint8_t* p = img + off * 3;
      v[0] = p[bgr ? 2 : 0]; v[1] = p[1]; v[2] = p[bgr ? 0 : 2];
    } else {
      v[0] = v[1] = v[2] = 0;
    }
  };
  auto pxd = [&](int r, int c) -> int {
    int64_t off;
    return (dimg && in_frame(r, c, off)) ? (int)dimg[off] : 0;
  };

  int outc[3];
  int dval = 0;
  float dvalf = 0.f;   // kFloatDepth: the unrounded depth in mm
  if (n == 2 * S) {
    // exact 2x downscale: cv::resize switches INTER_LINEAR to INTER_AREA (2x2 mean)
    const int r = 2 * oy, c = 2 * ox;
    int a[3], bq[3], cq[3], dq[3];
    px3(r, c, a); px3(r, c + 1, bq); px3(r + 1, c, cq); px3(r + 1, c + 1, dq);
#pragma unroll
    for (int k = 0; k < 3; ++k) outc[k] = (a[k] + bq[k] + cq[k] + dq[k] + 2) >> 2;
    if constexpr (kFloatDepth) {
      dvalf = (float)(pxd(r, c) + pxd(r, c + 1) + pxd(r + 1, c) + pxd(r + 1, c + 1)) * 0.25f;
    } else {
      dval = (pxd(r, c) + pxd(r, c + 1) + pxd(r + 1, c) + pxd(r + 1, c + 1) + 2) >> 2;
    }
  } else {
    int sx, sy;
    float fx, fy;
    lin_coef(ox, n, S, true, sx, fx);
    lin_coef(oy, n, S, false, sy, fy);
    const bool edge = sx >= n - 1;   // dx >= xmax: S[sx] * ONE
    const int c0 = sx, c1 = edge ? sx : sx + 1;
    const int r0 = sy < 0 ? 0 : (sy > n - 1 ? n - 1 : sy);
    const int r1 = sy + 1 < 0 ? 0 : (sy + 1 > n - 1 ? n - 1 : sy + 1);
    // 8U: HResizeLinear (int) + VResizeLinearVec_32s8u
    const int a0 = fix_coef(1.f - fx), a1 = fix_coef(fx);
    const int b0 = fix_coef(1.f - fy), b1 = fix_coef(fy);
    int p00[3], p01[3], p10[3], p11[3];
    px3(r0, c0, p00); px3(r0, c1, p01); px3(r1, c0, p10); px3(r1, c1, p11);
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      const int h0 = p00[k] * a0 + (edge ? 0 : p01[k] * a1);
      const int h1 = p10[k] * a0 + (edge ? 0 : p11[k] * a1);
      const int t = (((h0 >> 4) * b0) >> 16) + (((h1 >> 4) * b1) >> 16);
      const int v = (t + 2) >> 2;
      outc[k] = v < 0 ? 0 : (v > 255 ? 255 : v);
    }
    // 16U: float weights, mul + add, round half to even, saturate
    if (dimg) {
      const float fa0 = 1.f - fx, fb0 = 1.f - fy;
      const float d00 = (float)pxd(r0, c0), d10 = (float)pxd(r1, c0);
      const float h0 = edge ? d00 * 1.f : d00 * fa0 + (float)pxd(r0, c1) * fx;
      const float h1 = edge ? d10 * 1.f : d10 * fa0 + (float)pxd(r1, c1) * fx;
      if constexpr (kFloatDepth) {
        dvalf = h0 * fb0 + h1 * fy;
      } else {
        const float v = rintf(h0 * fb0 + h1 * fy);
        dval = v < 0.f ? 0 : (v > 65535.f ? 65535 : (int)v);
      }
    } else {
      dval = 0;
    }
  }

  // ToTensor (u8 / 255) + Normalize ((x - mean) / std), NCHW
  const int64_t plane = (int64_t)S * S;
  if (u8_out) {   // the resized uint8 crop, HWC (the PIL image ColorJitter receives)
    uint8_t* o = u8_out + ((int64_t)b * plane + pix) * 3;
    o[0] = (uint8_t)outc[0]; o[1] = (uint8_t)outc[1]; o[2] = (uint8_t)outc[2];
  }
  if (rgb_out) {
    float* o = rgb_out + (int64_t)b * 3 * plane + pix;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      float v = (float)outc[k] / 255.f;
      if (mean_std) v = (v - mean_std[k]) / mean_std[3 + k];
      o[k * plane] = v;
    }
  }
  // dataset_rgbd.py:176-186
  const float raw = (kFloatDepth ? dvalf : (float)dval) / 1000.f;
  if (depth_raw_out) depth_raw_out[(int64_t)b * plane + pix] = raw;
  if (depth_out) {
    float dn = (raw - 0.1f) / 1.5f;
    dn = fminf(fmaxf(dn, 0.f), 1.f);
    if (raw < 0.01f) dn = 0.f;
    depth_out[(int64_t)b * plane + pix] = dn;
  }
}

__global__ __launch_bounds__(kThreads) void crop_rgbd_kernel(
    const uint8_t* __restrict__ rgb, int bgr, const uint16_t* __restrict__ depth, int H, int W,
    const int32_t* __restrict__ bbox_orig, const int32_t* __restrict__ bbox_aug, const float* __restrict__ K, int S,
    const float* __restrict__ mean_std, float* __restrict__ rgb_out, float* __restrict__ depth_out,
    float* __restrict__ depth_raw_out, float* __restrict__ center_out, float* __restrict__ K_out,
    uint8_t* __restrict__ u8_out) {
  const int b = blockIdx.y;
  const int pix = blockIdx.x * kThreads + threadIdx.x;
  const int64_t HW = (int64_t)H * W;
  crop_pixel<false>(b, pix, rgb + (int64_t)b * HW * 3, bgr, depth ? depth + (int64_t)b * HW : nullptr, H, W,
             bbox_orig + 4 * b, bbox_aug + 4 * b, K + 9 * b, S, mean_std, rgb_out, depth_out, depth_raw_out,
             center_out, K_out, u8_out);
}

// The tables and the store of the indexed entry points (device pointers).
struct StoreTabs {
  const uint8_t* rgb;
  const uint16_t* depth;       // or nullptr
  int64_t n_frames, n_samples;
  const int32_t* frame_of;     // [n_samples]
  const int32_t* bbox;         // [n_samples][4]
  const float* K;              // [n_samples][9]
  const float* center;         // [n_samples][2] or nullptr
  const float* quat;           // [n_samples][4]
  const float* trans;          // [n_samples][3]
  const int64_t* obj_id;       // [n_samples]
};

struct LabelOuts {
  float* quat;
  float* trans;
  int64_t* obj;
  int32_t* status;
};

// Crop b of a batch drawn from a device-resident frame store: sample s = sample_idx[b]
// (read here, at kernel time), frame frame_of[s].  Nothing is read through an index
// before it has been range-checked: a bad sample or frame index zero-fills the crop's
// outputs, sets obj_out to -1 and raises *status to b + 1.  Otherwise crop_pixel on the
// sample's frame and table rows; the pix == 0 thread also gathers the labels (and, for
// the RGB datasets, the original-image centre and K).
__global__ __launch_bounds__(kThreads) void crop_rgbd_indexed_kernel(
    StoreTabs t, int bgr, int H, int W, const int64_t* __restrict__ sample_idx, const int32_t* __restrict__ bbox_aug,
    int S, const float* __restrict__ mean_std, float* __restrict__ rgb_out, float* __restrict__ depth_out,
    float* __restrict__ depth_raw_out, float* __restrict__ center_out, float* __restrict__ K_out, LabelOuts lab,
    uint8_t* __restrict__ u8_out) {
  const int b = blockIdx.y;
  const int pix = blockIdx.x * kThreads + threadIdx.x;
  const int64_t s = sample_idx[b];
  int64_t f = -1;
  if (s >= 0 && s < t.n_samples) f = (int64_t)t.frame_of[s];
  const int64_t plane = (int64_t)S * S;
  if (f < 0 || f >= t.n_frames) {   // also: s out of range (f stayed -1)
    if (pix == 0) {
      if (center_out) center_out[2 * b] = center_out[2 * b + 1] = 0.f;
      if (K_out)
        for (int i = 0; i < 9; ++i) K_out[9 * b + i] = 0.f;
      if (lab.quat)
        for (int i = 0; i < 4; ++i) lab.quat[4 * b + i] = 0.f;
      if (lab.trans)
        for (int i = 0; i < 3; ++i) lab.trans[3 * b + i] = 0.f;
      if (lab.obj) lab.obj[b] = -1;
      if (lab.status) atomicMax(lab.status, b + 1);
    }
    if (pix >= plane) return;
    if (u8_out) {
      uint8_t* o = u8_out + ((int64_t)b * plane + pix) * 3;
      o[0] = o[1] = o[2] = 0;
    }
    if (rgb_out)
      for (int k = 0; k < 3; ++k) rgb_out[((int64_t)b * 3 + k) * plane + pix] = 0.f;
    if (depth_raw_out) depth_raw_out[(int64_t)b * plane + pix] = 0.f;
    if (depth_out) depth_out[(int64_t)b * plane + pix] = 0.f;
    return;
  }
  if (pix == 0) {
    if (lab.quat)
      for (int i = 0; i < 4; ++i) lab.quat[4 * b + i] = t.quat[4 * s + i];
    if (lab.trans)
      for (int i = 0; i < 3; ++i) lab.trans[3 * b + i] = t.trans[3 * s + i];
    if (lab.obj) lab.obj[b] = t.obj_id[s];
    if (t.center) {   // dataset_rgb.py:96,139-141: the original-image centre and K, as stored
      if (center_out) { center_out[2 * b] = t.center[2 * s]; center_out[2 * b + 1] = t.center[2 * s + 1]; }
      if (K_out)
        for (int i = 0; i < 9; ++i) K_out[9 * b + i] = t.K[9 * s + i];
    }
  }
  const int64_t HW = (int64_t)H * W;
  const int32_t* bo = t.bbox + 4 * s;
  crop_pixel<false>(b, pix, t.rgb + f * HW * 3, bgr, t.depth ? t.depth + f * HW : nullptr, H, W, bo,
             bbox_aug ? bbox_aug + 4 * b : bo, t.K + 9 * s, S, mean_std, rgb_out, depth_out, depth_raw_out,
             t.center ? nullptr : center_out, t.center ? nullptr : K_out, u8_out);
}

// The small per-detection outputs of the inference path.
struct DetOuts {
  float* center_crop;   // [N][2]
  float* K_crop;        // [N][9]
  float* center_img;    // [N][2]
  float* K_img;         // [N][9]
  int32_t* status;
};

// Detection b of N over F frames: the per-detection body of the reference's inference
// scripts (inference_rgbd_geometric.py:110-182) up to the model call.  The box is
// (x1, y1, x2, y2), read here at kernel time; its square crop is crop_geom on
// (x1, y1, x2 - x1, y2 - y1) (:118-135: (x1 + x2) / 2 and x1 + (x2 - x1) / 2 are both
// exact in double).  The pixels are crop_pixel's with the float depth flavour; the centre
// and intrinsics run in double and round once (:145-167), unlike the dataset's float32.
__global__ __launch_bounds__(kThreads) void crop_detections_kernel(
    const uint8_t* __restrict__ frames, int bgr, const uint16_t* __restrict__ depth, int F, int H, int W,
    const int32_t* __restrict__ frame_of, const int32_t* __restrict__ boxes, const double* __restrict__ K,
    int K_per_frame, int S, const float* __restrict__ mean_std, int k_mode, float* __restrict__ rgb_out,
    float* __restrict__ depth_out, float* __restrict__ depth_raw_out, DetOuts o) {
  const int b = blockIdx.y;
  const int pix = blockIdx.x * kThreads + threadIdx.x;
  const int f = frame_of ? frame_of[b] : 0;
  const int64_t plane = (int64_t)S * S;
  if (f < 0 || f >= F) {   // nothing is read through the bad index
    if (pix == 0) {
      if (o.center_crop) o.center_crop[2 * b] = o.center_crop[2 * b + 1] = 0.f;
      if (o.center_img) o.center_img[2 * b] = o.center_img[2 * b + 1] = 0.f;
      for (int i = 0; i < 9; ++i) {
        if (o.K_crop) o.K_crop[9 * b + i] = 0.f;
        if (o.K_img) o.K_img[9 * b + i] = 0.f;
      }
      if (o.status) atomicMax(o.status, b + 1);
    }
    if (pix >= plane) return;
    if (rgb_out)
      for (int k = 0; k < 3; ++k) rgb_out[((int64_t)b * 3 + k) * plane + pix] = 0.f;
    if (depth_raw_out) depth_raw_out[(int64_t)b * plane + pix] = 0.f;
    if (depth_out) depth_out[(int64_t)b * plane + pix] = 0.f;
    return;
  }
  const int32_t* bx = boxes + 4 * b;
  const int32_t bb[4] = {bx[0], bx[1], bx[2] - bx[0], bx[3] - bx[1]};
  if (pix == 0) {
    const CropGeom g = crop_geom(bb, H, W);
    const double* k = K + (K_per_frame ? 9 * (int64_t)f : 0);
    const double c_x = ((double)bx[0] + (double)bx[2]) / 2.0, c_y = ((double)bx[1] + (double)bx[3]) / 2.0;
    const double scale = (double)S / (double)g.n;
    if (o.center_crop) {   // :145-153: double, one cast, then the clip on the float32 array
      const float ccx = (float)(((c_x + (double)g.pad_l) - (double)(g.x1 + g.pad_l)) * scale);
      const float ccy = (float)(((c_y + (double)g.pad_t) - (double)(g.y1 + g.pad_t)) * scale);
      o.center_crop[2 * b] = fminf(fmaxf(ccx, 0.f), (float)(S - 1));
      o.center_crop[2 * b + 1] = fminf(fmaxf(ccy, 0.f), (float)(S - 1));
    }
    if (o.K_crop) {
      // k_mode 0, :156-167: the script subtracts the UNPADDED origin after adding the pad,
      // pad_l * scale more than k_mode 1, the dataset's (cx + pad_l - (x1 + pad_l)) =
      // (cx - x1) * scale (dataset_rgbd.py:159-169) that the model was trained on
      const double ox = k_mode ? k[2] - (double)g.x1 : (k[2] + (double)g.pad_l) - (double)g.x1;
      const double oy = k_mode ? k[5] - (double)g.y1 : (k[5] + (double)g.pad_t) - (double)g.y1;
      float* ko = o.K_crop + 9 * b;
      ko[0] = (float)(k[0] * scale); ko[1] = 0.f; ko[2] = (float)(ox * scale);
      ko[3] = 0.f; ko[4] = (float)(k[4] * scale); ko[5] = (float)(oy * scale);
      ko[6] = 0.f; ko[7] = 0.f; ko[8] = 1.f;
    }
    if (o.center_img) {   // inference_rgb_geometric.py:105-106
      o.center_img[2 * b] = (float)c_x;
      o.center_img[2 * b + 1] = (float)c_y;
    }
    if (o.K_img)
      for (int i = 0; i < 9; ++i) o.K_img[9 * b + i] = (float)k[i];
  }
  const int64_t HW = (int64_t)H * W;
  crop_pixel<true>(b, pix, frames + (int64_t)f * HW * 3, bgr, depth ? depth + (int64_t)f * HW : nullptr, H, W, bb, bb,
                   nullptr, S, mean_std, rgb_out, depth_out, depth_raw_out, nullptr, nullptr, nullptr);
}

}  // namespace

extern "C" int pose6d_crop_detections(const uint8_t* frames, int32_t bgr, const uint16_t* depth, int32_t F, int32_t H,
                                      int32_t W, const int32_t* frame_of, const int32_t* boxes_xyxy, int32_t N,
                                      const double* K, int32_t K_per_frame, int32_t S, const float* mean_std,
                                      int32_t k_mode, float* rgb_out, float* depth_out, float* depth_raw_out,
                                      float* center_crop_out, float* K_crop_out, float* center_img_out,
                                      float* K_img_out, int32_t* status, void* stream) {
  P6_CHECK_ARG(frames != nullptr && boxes_xyxy != nullptr, "pose6d_crop_detections: frames and boxes_xyxy are required");
  P6_CHECK_ARG(N >= 0 && N <= 65535 && F > 0 && H > 0 && W > 0 && S > 0 && (int64_t)S * S < (1ll << 31),
               "pose6d_crop_detections: bad shape");
  P6_CHECK_ARG((K_crop_out == nullptr && K_img_out == nullptr) || K != nullptr,
               "pose6d_crop_detections: K_crop_out / K_img_out need K");
  P6_CHECK_ARG(k_mode == 0 || k_mode == 1, "pose6d_crop_detections: k_mode is 0 (script) or 1 (dataset)");
  if (N == 0) return POSE6D_OK;
  const DetOuts o{center_crop_out, K_crop_out, center_img_out, K_img_out, status};
  const dim3 grid(p6::ceil_div((int64_t)S * S, kThreads), N);
  crop_detections_kernel<<<grid, kThreads, 0, p6::stream_of(stream)>>>(frames, bgr, depth, F, H, W, frame_of,
                                                                       boxes_xyxy, K, K_per_frame, S, mean_std, k_mode,
                                                                       rgb_out, depth_out, depth_raw_out, o);
  P6_LAUNCH_CHECK();
  return POSE6D_OK;
}

extern "C" int pose6d_crop_rgbd(const uint8_t* rgb, int32_t bgr, const uint16_t* depth, int32_t B, int32_t H,
                                int32_t W, const int32_t* bbox_orig, const int32_t* bbox_aug, const float* K,
                                int32_t S, const float* mean_std, float* rgb_out, float* depth_out,
                                float* depth_raw_out, float* center_out, float* K_out, void* stream) {
  P6_CHECK_ARG(rgb != nullptr && bbox_aug != nullptr, "pose6d_crop_rgbd: rgb and bbox_aug are required");
  P6_CHECK_ARG(B >= 0 && H > 0 && W > 0 && S > 0 && (int64_t)S * S < (1ll << 31), "pose6d_crop_rgbd: bad shape");
  P6_CHECK_ARG(center_out == nullptr || bbox_orig != nullptr, "pose6d_crop_rgbd: center_out needs bbox_orig");
  P6_CHECK_ARG(K_out == nullptr || K != nullptr, "pose6d_crop_rgbd: K_out needs K");
  if (B == 0) return POSE6D_OK;
  const dim3 grid(p6::ceil_div((int64_t)S * S, kThreads), B);
  crop_rgbd_kernel<<<grid, kThreads, 0, p6::stream_of(stream)>>>(rgb, bgr, depth, H, W, bbox_orig, bbox_aug, K, S,
                                                                 mean_std, rgb_out, depth_out, depth_raw_out,
                                                                 center_out, K_out, nullptr);
  P6_LAUNCH_CHECK();
  return POSE6D_OK;
}

// The argument checks the two indexed entry points share (`fn`: the name in the message).
#define P6_CHECK_INDEXED_ARGS(fn)                                                                                  \
  P6_CHECK_ARG(rgb_store != nullptr && frame_of != nullptr && bbox != nullptr && K != nullptr && quat != nullptr && \
                   trans != nullptr && obj_id != nullptr && sample_idx != nullptr,                                  \
               fn ": rgb_store, the tables (frame_of, bbox, K, quat, trans, obj_id) and sample_idx are required");  \
  P6_CHECK_ARG(B >= 0 && B <= 65535 && n_samples >= 0 && n_frames >= 0 && n_samples < (1ll << 31) &&                \
                   n_frames < (1ll << 31) && H > 0 && W > 0 && S > 0 && (int64_t)S * S < (1ll << 31),               \
               fn ": bad shape");                                                                                   \
  P6_CHECK_ARG(K_out == nullptr || K != nullptr, fn ": K_out needs K");                                            \
  P6_CHECK_ARG(center_out == nullptr || center_tab != nullptr || bbox != nullptr,                                  \
               fn ": center_out needs center_tab or bbox")

extern "C" int pose6d_crop_rgbd_indexed(const uint8_t* rgb_store, int32_t bgr, const uint16_t* depth_store,
                                        int64_t n_frames, int32_t H, int32_t W, const int32_t* frame_of,
                                        const int32_t* bbox, const float* K, const float* center_tab,
                                        const float* quat, const float* trans, const int64_t* obj_id,
                                        int64_t n_samples, const int64_t* sample_idx, const int32_t* bbox_aug,
                                        int32_t B, int32_t S, const float* mean_std, float* rgb_out,
                                        float* depth_out, float* depth_raw_out, float* center_out, float* K_out,
                                        float* quat_out, float* trans_out, int64_t* obj_out, int32_t* status,
                                        void* stream) {
  P6_CHECK_INDEXED_ARGS("pose6d_crop_rgbd_indexed");
  if (B == 0) return POSE6D_OK;
  const StoreTabs t{rgb_store, depth_store, n_frames, n_samples, frame_of, bbox, K, center_tab, quat, trans, obj_id};
  const LabelOuts lab{quat_out, trans_out, obj_out, status};
  const dim3 grid(p6::ceil_div((int64_t)S * S, kThreads), B);
  crop_rgbd_indexed_kernel<<<grid, kThreads, 0, p6::stream_of(stream)>>>(
      t, bgr, H, W, sample_idx, bbox_aug, S, mean_std, rgb_out, depth_out, depth_raw_out, center_out, K_out, lab,
      nullptr);
  P6_LAUNCH_CHECK();
  return POSE6D_OK;
}

// ---------------------------------------------------------------- train transform
// The reference's train_transform (train_rgbd_geometric.py:41-47) on the resized
// uint8 crop: ColorJitter(brightness, contrast, saturation, hue) in a random op order
// -> ToTensor -> Normalize -> RandomErasing(p, scale, ratio, value 0).  ColorJitter's
// arithmetic is Pillow's (torchvision applies it to a PIL image): ImageEnhance =
// Image.blend against a degenerate image (black / the constant int(mean L + 0.5) /
// the L image), float alpha, truncating; hue through Pillow's HSV conversion with
// torchvision's uint8 hue-band shift -- restated in oracle/augment.py and pinned there
// against Pillow itself.  One 1024-thread workgroup per crop holds the crop in LDS
// (S * S * 3 bytes: 147 KiB at 224) while the four ops run in place, the contrast
// mean being a workgroup reduction of the current image.
// Random parameters: counter-based draws (splitmix64 of seed, crop, draw index) with
// torchvision's distributions (get_params of ColorJitter / RandomErasing); every
// crop's parameters are written to params_out so a checker can replay them.
namespace {

constexpr int kAugThreads = 1024;
constexpr int kAugParams = 16;   // perm[4], factor[4] (NaN: op off), erase i, j, h, w (-1: none), 4 spare

struct AugCfg {
  float lo[4], hi[4];   // brightness, contrast, saturation, hue ranges (lo == hi == NaN: off)
  float p, scale_lo, scale_hi, log_r_lo, log_r_hi;
};

__device__ __forceinline__ uint64_t splitmix(uint64_t x) {
  x += 0x9E3779B97F4A7C15ull;
  x = (x ^ (x >> 30)) * 0xBF58476D1CE4E5B9ull;
  x = (x ^ (x >> 27)) * 0x94D049BB133111EBull;
  return x ^ (x >> 31);
}

// draw k of crop b: a uniform double in [0, 1)
__device__ __forceinline__ double u01(uint64_t seed, int b, int k) {
  const uint64_t x = splitmix(seed ^ splitmix(((uint64_t)(uint32_t)b << 32) | (uint32_t)k));
  return (double)(x >> 11) * 0x1.0p-53;
}

// a float32 tensor's uniform_(lo, hi) value
__device__ __forceinline__ float uf(uint64_t seed, int b, int k, float lo, float hi) {
  return (float)((double)lo + ((double)hi - (double)lo) * u01(seed, b, k));
}

// Pillow ImagingBlend on one uint8 band value
__device__ __forceinline__ int blend_u8(int d, int v, float a) {
  if (a == 0.f) return d;
  if (a == 1.f) return v;
  const float t = (float)d + a * (float)(v - d);
  if (a >= 0.f && a <= 1.f) return (int)(uint8_t)t;
  return t <= 0.f ? 0 : (t >= 255.f ? 255 : (int)(uint8_t)t);
}

__device__ __forceinline__ int lum_u8(int r, int g, int b) { return (r * 19595 + g * 38470 + b * 7471 + 0x8000) >> 16; }

__device__ __forceinline__ int clip8(int v) { return v < 0 ? 0 : (v > 255 ? 255 : v); }

// Pillow rgb2hsv_row / hsv2rgb (oracle/augment.py spells out the rounding of each step)
__device__ __forceinline__ void rgb2hsv(int r, int g, int b, int& h8, int& s8, int& v8) {
  const int maxc = max(r, max(g, b)), minc = min(r, min(g, b));
  v8 = maxc;
  if (maxc == minc) { h8 = 0; s8 = 0; return; }
  const float cr = (float)(maxc - minc);
  const float s = cr / (float)maxc;
  const float rc = (float)(maxc - r) / cr, gc = (float)(maxc - g) / cr, bc = (float)(maxc - b) / cr;
  float h;
  if (r == maxc) h = bc - gc;
  else if (g == maxc) h = (float)(2.0 + (double)rc - (double)bc);
  else h = (float)(4.0 + (double)gc - (double)rc);
  h = (float)fmod((double)h / 6.0 + 1.0, 1.0);
  h8 = clip8((int)((double)h * 255.0));
  s8 = clip8((int)((double)s * 255.0));
}

__device__ __forceinline__ void hsv2rgb(int h8, int s8, int v8, int& r, int& g, int& b) {
  if (s8 == 0) { r = g = b = v8; return; }
  const double hf = (double)(float)h8;
  const double i = floor(hf * 6.0 / 255.0);
  const double f = (double)(float)(hf * 6.0 / 255.0 - i);
  const double fs = (double)(float)((double)(float)s8 / 255.0);
  const double vf = (double)(float)v8;
  const int p = clip8((int)round(vf * (1.0 - fs)));
  const int q = clip8((int)round(vf * (1.0 - fs * f)));
  const int t = clip8((int)round(vf * (1.0 - fs * (1.0 - f))));
  switch ((int)i % 6) {
    case 0: r = v8; g = t; b = p; break;
    case 1: r = q; g = v8; b = p; break;
    case 2: r = p; g = v8; b = t; break;
    case 3: r = p; g = q; b = v8; break;
    case 4: r = t; g = p; b = v8; break;
    default: r = v8; g = p; b = q; break;
  }
}

__global__ __launch_bounds__(kAugThreads) void augment_kernel(const uint8_t* __restrict__ src, int S,
                                                              const float* __restrict__ mean_std, AugCfg cfg,
                                                              uint64_t seed, const uint64_t* __restrict__ seed_dev,
                                                              float* __restrict__ rgb_out,
                                                              float* __restrict__ params_out) {
  extern __shared__ __attribute__((aligned(16))) uint8_t img[];   // [S][S][3]
  if (seed_dev) seed = *seed_dev;   // the device-seed entry point: read now, uniform over the launch
  __shared__ int red[kAugThreads / 64];
  __shared__ float prm[kAugParams];
  const int b = blockIdx.x, tid = threadIdx.x;
  const int npx = S * S, nbytes = npx * 3;
  const uint8_t* in = src + (int64_t)b * nbytes;
  for (int i = tid * 16; i < nbytes; i += kAugThreads * 16) {
    if (i + 16 <= nbytes) {
      *reinterpret_cast<uint4*>(img + i) = *reinterpret_cast<const uint4*>(in + i);
    } else {
      for (int k = i; k < nbytes; ++k) img[k] = in[k];
    }
  }
  if (tid == 0) {
    // ColorJitter.get_params: fn_idx = randperm(4), then each enabled factor
    int perm[4] = {0, 1, 2, 3};
    for (int i = 3; i > 0; --i) {   // Fisher-Yates
      const int j = (int)(u01(seed, b, 3 - i) * (double)(i + 1));
      const int t = perm[i]; perm[i] = perm[j]; perm[j] = t;
    }
    for (int k = 0; k < 4; ++k) {
      prm[k] = (float)perm[k];
      prm[4 + k] = isnan(cfg.lo[k]) ? cfg.lo[k] : uf(seed, b, 3 + k, cfg.lo[k], cfg.hi[k]);
    }
    // RandomErasing.forward / get_params (value 0): p, then up to 10 attempts
    float box[4] = {-1.f, -1.f, -1.f, -1.f};
    if (u01(seed, b, 7) < (double)cfg.p) {
      const double area = (double)S * (double)S;
      for (int att = 0; att < 10; ++att) {
        const int k0 = 8 + 4 * att;
        const double ea = area * (double)uf(seed, b, k0, cfg.scale_lo, cfg.scale_hi);
        const double ar = (double)expf(uf(seed, b, k0 + 1, cfg.log_r_lo, cfg.log_r_hi));
        const int h = (int)rint(sqrt(ea * ar)), w = (int)rint(sqrt(ea / ar));   // round(): half to even
        if (!(h < S && w < S)) continue;
        box[0] = (float)(int)(u01(seed, b, k0 + 2) * (double)(S - h + 1));
        box[1] = (float)(int)(u01(seed, b, k0 + 3) * (double)(S - w + 1));
        box[2] = (float)h;
        box[3] = (float)w;
        break;
      }
    }
    for (int k = 0; k < 4; ++k) prm[8 + k] = box[k];
    for (int k = 12; k < kAugParams; ++k) prm[k] = 0.f;
    if (params_out)
      for (int k = 0; k < kAugParams; ++k) params_out[b * kAugParams + k] = prm[k];
  }
  __syncthreads();
  for (int step = 0; step < 4; ++step) {
    const int op = (int)prm[step];
    const float f = prm[4 + op];
    if (isnan(f)) continue;   // op disabled (block-uniform)
    int mean = 0;
    if (op == 1) {            // contrast: int(mean(L) + 0.5) of the current image
      int sum = 0;
      for (int p = tid; p < npx; p += kAugThreads) sum += lum_u8(img[3 * p], img[3 * p + 1], img[3 * p + 2]);
      sum = p6::wave_sum(sum);
      if ((tid & 63) == 0) red[tid >> 6] = sum;
      __syncthreads();
      int tot = 0;
#pragma unroll
      for (int w = 0; w < kAugThreads / 64; ++w) tot += red[w];
      mean = (int)((double)tot / (double)npx + 0.5);
    }
    const int shift = op == 3 ? ((int)(int8_t)(int)((double)f * 255.0) & 255) : 0;
    for (int p = tid; p < npx; p += kAugThreads) {
      int r = img[3 * p], g = img[3 * p + 1], bl = img[3 * p + 2];
      if (op == 0) {
        r = blend_u8(0, r, f); g = blend_u8(0, g, f); bl = blend_u8(0, bl, f);
      } else if (op == 1) {
        r = blend_u8(mean, r, f); g = blend_u8(mean, g, f); bl = blend_u8(mean, bl, f);
      } else if (op == 2) {
        const int l = lum_u8(r, g, bl);
        r = blend_u8(l, r, f); g = blend_u8(l, g, f); bl = blend_u8(l, bl, f);
      } else {
        int h8, s8, v8;
        rgb2hsv(r, g, bl, h8, s8, v8);
        hsv2rgb((h8 + shift) & 255, s8, v8, r, g, bl);
      }
      img[3 * p] = (uint8_t)r; img[3 * p + 1] = (uint8_t)g; img[3 * p + 2] = (uint8_t)bl;
    }
    __syncthreads();
  }
  // ToTensor + Normalize + RandomErasing (value 0), NCHW fp32, coalesced along x
  const int bi = (int)prm[8], bj = (int)prm[9], bh = (int)prm[10], bw = (int)prm[11];
  float* o = rgb_out + (int64_t)b * 3 * npx;
  for (int p = tid; p < npx; p += kAugThreads) {
    const int y = p / S, x = p - y * S;
    const bool erased = bh > 0 && y >= bi && y < bi + bh && x >= bj && x < bj + bw;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      float v = (float)img[3 * p + k] / 255.f;
      if (mean_std) v = (v - mean_std[k]) / mean_std[3 + k];
      o[(int64_t)k * npx + p] = erased ? 0.f : v;
    }
  }
}

}  // namespace

namespace {

#define P6_CHECK_AUG_ARGS(fn)                                                                                   \
  P6_CHECK_ARG(brightness >= 0.f && contrast >= 0.f && saturation >= 0.f && hue >= 0.f && hue <= 0.5f,           \
               fn ": ColorJitter factors must be >= 0 (hue <= 0.5)");                                            \
  P6_CHECK_ARG(erase_p >= 0.f && erase_p <= 1.f && erase_scale_lo <= erase_scale_hi && erase_ratio_lo > 0.f &&   \
                   erase_ratio_lo <= erase_ratio_hi,                                                             \
               fn ": bad RandomErasing arguments")

// ColorJitter._check_input: value v -> [max(0, 1 - v), 1 + v] (hue: [-v, v]); 0 -> the op is off
AugCfg aug_cfg(float brightness, float contrast, float saturation, float hue, float erase_p, float erase_scale_lo,
               float erase_scale_hi, float erase_ratio_lo, float erase_ratio_hi) {
  AugCfg cfg;
  const float v[4] = {brightness, contrast, saturation, hue};
  for (int k = 0; k < 4; ++k) {
    if (v[k] == 0.f) {
      cfg.lo[k] = cfg.hi[k] = __builtin_nanf("");
    } else if (k == 3) {
      cfg.lo[k] = -v[k]; cfg.hi[k] = v[k];
    } else {
      cfg.lo[k] = 1.f - v[k] > 0.f ? 1.f - v[k] : 0.f; cfg.hi[k] = 1.f + v[k];
    }
  }
  cfg.p = erase_p;
  cfg.scale_lo = erase_scale_lo;
  cfg.scale_hi = erase_scale_hi;
  cfg.log_r_lo = logf(erase_ratio_lo);   // torch.log(torch.tensor(ratio)): float32
  cfg.log_r_hi = logf(erase_ratio_hi);
  return cfg;
}

}  // namespace

extern "C" int64_t pose6d_crop_train_workspace(int32_t B, int32_t S) { return (int64_t)B * S * S * 3; }

extern "C" int pose6d_crop_rgbd_train(const uint8_t* rgb, int32_t bgr, const uint16_t* depth, int32_t B, int32_t H,
                                      int32_t W, const int32_t* bbox_orig, const int32_t* bbox_aug, const float* K,
                                      int32_t S, const float* mean_std, float brightness, float contrast,
                                      float saturation, float hue, float erase_p, float erase_scale_lo,
                                      float erase_scale_hi, float erase_ratio_lo, float erase_ratio_hi,
                                      uint64_t seed, uint8_t* workspace, float* rgb_out, float* depth_out,
                                      float* depth_raw_out, float* center_out, float* K_out, float* params_out,
                                      void* stream) {
  P6_CHECK_ARG(rgb != nullptr && bbox_aug != nullptr && workspace != nullptr && rgb_out != nullptr,
               "pose6d_crop_rgbd_train: rgb, bbox_aug, workspace and rgb_out are required");
  P6_CHECK_ARG(B >= 0 && H > 0 && W > 0 && S > 0 && S <= 232, "pose6d_crop_rgbd_train: bad shape (S <= 232: the "
               "crop must fit one workgroup's LDS)");
  P6_CHECK_ARG(center_out == nullptr || bbox_orig != nullptr, "pose6d_crop_rgbd_train: center_out needs bbox_orig");
  P6_CHECK_ARG(K_out == nullptr || K != nullptr, "pose6d_crop_rgbd_train: K_out needs K");
  P6_CHECK_AUG_ARGS("pose6d_crop_rgbd_train");
  if (B == 0) return POSE6D_OK;
  hipStream_t s = p6::stream_of(stream);
  const dim3 grid(p6::ceil_div((int64_t)S * S, kThreads), B);
  crop_rgbd_kernel<<<grid, kThreads, 0, s>>>(rgb, bgr, depth, H, W, bbox_orig, bbox_aug, K, S, nullptr, nullptr,
                                             depth_out, depth_raw_out, center_out, K_out, workspace);
  P6_LAUNCH_CHECK();
  const AugCfg cfg = aug_cfg(brightness, contrast, saturation, hue, erase_p, erase_scale_lo, erase_scale_hi,
                             erase_ratio_lo, erase_ratio_hi);
  augment_kernel<<<B, kAugThreads, S * S * 3, s>>>(workspace, S, mean_std, cfg, seed, nullptr, rgb_out, params_out);
  P6_LAUNCH_CHECK();
  return POSE6D_OK;
}

namespace {

// The two launches of the indexed train crop: `seed` by value, or read from seed_dev at
// kernel time when that is given.
int launch_train_indexed(const StoreTabs& t, int bgr, int H, int W, const int64_t* sample_idx, const int32_t* bbox_aug,
                         int B, int S, const float* mean_std, const AugCfg& cfg, uint64_t seed,
                         const uint64_t* seed_dev, uint8_t* workspace, float* rgb_out, float* depth_out,
                         float* depth_raw_out, float* center_out, float* K_out, const LabelOuts& lab,
                         float* params_out, hipStream_t s) {
  const dim3 grid(p6::ceil_div((int64_t)S * S, kThreads), B);
  crop_rgbd_indexed_kernel<<<grid, kThreads, 0, s>>>(t, bgr, H, W, sample_idx, bbox_aug, S, nullptr, nullptr,
                                                     depth_out, depth_raw_out, center_out, K_out, lab, workspace);
  P6_LAUNCH_CHECK();
  augment_kernel<<<B, kAugThreads, S * S * 3, s>>>(workspace, S, mean_std, cfg, seed, seed_dev, rgb_out, params_out);
  P6_LAUNCH_CHECK();
  return POSE6D_OK;
}

}  // namespace

extern "C" int pose6d_crop_rgbd_train_indexed(
    const uint8_t* rgb_store, int32_t bgr, const uint16_t* depth_store, int64_t n_frames, int32_t H, int32_t W,
    const int32_t* frame_of, const int32_t* bbox, const float* K, const float* center_tab, const float* quat,
    const float* trans, const int64_t* obj_id, int64_t n_samples, const int64_t* sample_idx, const int32_t* bbox_aug,
    int32_t B, int32_t S, const float* mean_std, float brightness, float contrast, float saturation, float hue,
    float erase_p, float erase_scale_lo, float erase_scale_hi, float erase_ratio_lo, float erase_ratio_hi,
    uint64_t seed, uint8_t* workspace, float* rgb_out, float* depth_out, float* depth_raw_out, float* center_out,
    float* K_out, float* quat_out, float* trans_out, int64_t* obj_out, float* params_out, int32_t* status,
    void* stream) {
  P6_CHECK_INDEXED_ARGS("pose6d_crop_rgbd_train_indexed");
  P6_CHECK_ARG(workspace != nullptr && rgb_out != nullptr,
               "pose6d_crop_rgbd_train_indexed: workspace and rgb_out are required");
  P6_CHECK_ARG(S <= 232, "pose6d_crop_rgbd_train_indexed: bad shape (S <= 232: the crop must fit one workgroup's "
               "LDS)");
  P6_CHECK_AUG_ARGS("pose6d_crop_rgbd_train_indexed");
  if (B == 0) return POSE6D_OK;
  const StoreTabs t{rgb_store, depth_store, n_frames, n_samples, frame_of, bbox, K, center_tab, quat, trans, obj_id};
  const LabelOuts lab{quat_out, trans_out, obj_out, status};
  const AugCfg cfg = aug_cfg(brightness, contrast, saturation, hue, erase_p, erase_scale_lo, erase_scale_hi,
                             erase_ratio_lo, erase_ratio_hi);
  return launch_train_indexed(t, bgr, H, W, sample_idx, bbox_aug, B, S, mean_std, cfg, seed, nullptr, workspace,
                              rgb_out, depth_out, depth_raw_out, center_out, K_out, lab, params_out,
                              p6::stream_of(stream));
}

extern "C" int pose6d_crop_rgbd_train_indexed_dseed(
    const uint8_t* rgb_store, int32_t bgr, const uint16_t* depth_store, int64_t n_frames, int32_t H, int32_t W,
    const int32_t* frame_of, const int32_t* bbox, const float* K, const float* center_tab, const float* quat,
    const float* trans, const int64_t* obj_id, int64_t n_samples, const int64_t* sample_idx, const int32_t* bbox_aug,
    int32_t B, int32_t S, const float* mean_std, float brightness, float contrast, float saturation, float hue,
    float erase_p, float erase_scale_lo, float erase_scale_hi, float erase_ratio_lo, float erase_ratio_hi,
    const uint64_t* seed, uint8_t* workspace, float* rgb_out, float* depth_out, float* depth_raw_out,
    float* center_out, float* K_out, float* quat_out, float* trans_out, int64_t* obj_out, float* params_out,
    int32_t* status, void* stream) {
  P6_CHECK_INDEXED_ARGS("pose6d_crop_rgbd_train_indexed_dseed");
  P6_CHECK_ARG(workspace != nullptr && rgb_out != nullptr && seed != nullptr,
               "pose6d_crop_rgbd_train_indexed_dseed: workspace, rgb_out and seed are required");
  P6_CHECK_ARG(S <= 232, "pose6d_crop_rgbd_train_indexed_dseed: bad shape (S <= 232: the crop must fit one "
               "workgroup's LDS)");
  P6_CHECK_AUG_ARGS("pose6d_crop_rgbd_train_indexed_dseed");
  if (B == 0) return POSE6D_OK;
  const StoreTabs t{rgb_store, depth_store, n_frames, n_samples, frame_of, bbox, K, center_tab, quat, trans, obj_id};
  const LabelOuts lab{quat_out, trans_out, obj_out, status};
  const AugCfg cfg = aug_cfg(brightness, contrast, saturation, hue, erase_p, erase_scale_lo, erase_scale_hi,
                             erase_ratio_lo, erase_ratio_hi);
  return launch_train_indexed(t, bgr, H, W, sample_idx, bbox_aug, B, S, mean_std, cfg, 0, seed, workspace, rgb_out,
                              depth_out, depth_raw_out, center_out, K_out, lab, params_out, p6::stream_of(stream));
}
