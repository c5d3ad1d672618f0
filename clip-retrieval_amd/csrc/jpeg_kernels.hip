// jpeg_kernels.hip -- the pixel stage of the GPU JPEG decoder, bit-identical to Pillow / libjpeg's default decode.
//
// The entropy stage (jpegx_entropy.h, host) leaves int16 DCT coefficients; everything behind it is integer arithmetic on the
// VALU (no MFMA: an 8 x 8 integer butterfly with libjpeg's rounding is not a matrix product any matrix core computes exactly):
//   idct_kernel   coefficients -> u8 sample planes at component resolution, padded to whole blocks.  Dequantise, then libjpeg's
//                 slow-integer inverse DCT (jidctint: 13 constant bits, 2 extra bits kept after the column pass, descale by
//                 13 + 2 + 3 after the row pass, + 128, limited to 0 .. 255).  One wave = 8 blocks: a lane loads one ROW of a
//                 block (16 bytes), the transposition to "one lane per column" and back goes through the LDS.
//   rgb_kernel    planes -> packed RGB.  Chroma "fancy" (triangle) upsampling as jdsample does it -- 2x1: (3a + b + 1) >> 2 /
//                 (3a + b + 2) >> 2; 2x2: vertical 3a + b first, then (3s + t + 8) >> 4 / (3s + t + 7) >> 4 -- with the first / last
//                 column and row replicated from the REAL extent ceil(w / 2) x ceil(h / 2), plain replication when that width is
//                 <= 2; then JFIF YCbCr -> RGB in 16-bit fixed point.  Only the h x w real pixels are written.
// HBM traffic per pixel (4:2:0): 3 B coefficients + 1.5 B planes written + 1.5 B read (mostly from L2) + 3 B RGB.

#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string.h>
#include <algorithm>
#include <mutex>
#include <string>
#include <vector>

#include "../../include/clipx.h"
#include "clipx_host.h"
#include "clipx_upload_ring.h"
#include "jpegx_entropy.h"

static_assert(sizeof(clipx_jpeg_desc) == sizeof(jpegx::Desc), "clipx_jpeg_desc is jpegx::Desc");

namespace {

struct JImg {             // one per image, in the table buffer
  long long coef_off;     // byte offset of the record (quantisation tables, then coefficients) in the coefficient buffer
  long long plane_off;    // byte offset of component 0's plane in the plane scratch
  long long pix_off;      // byte offset of the RGB image in the packed pixel buffer
  int w, h, ncomp, hs, vs;
  int bw[3], bh[3];
  int blocks;
  int nb01[2];            // blocks of component 0, of components 0 + 1
  int pad;
};
static_assert(sizeof(JImg) % 8 == 0, "descriptors are read as an array");

__device__ __forceinline__ int limit8(int v) {
  v = v < 0 ? 0 : (v > 255 ? 255 : v);
  asm volatile("" : "+v"(v));  // kept opaque like preprocess.hip's clip8: no fused shift-saturate-pack of two results
  return v;
}

constexpr int CONST_BITS = 13, PASS1_BITS = 2;
constexpr int F_0_298 = 2446, F_0_390 = 3196, F_0_541 = 4433, F_0_765 = 6270, F_0_899 = 7373, F_1_175 = 9633, F_1_501 = 12299,
              F_1_847 = 15137, F_1_961 = 16069, F_2_053 = 16819, F_2_562 = 20995, F_3_072 = 25172;

// jidctint's 1-D pass on eight values, in place; `shift` is the (rounded) descale of the pass
__device__ __forceinline__ void idct8(int* v, int shift) {
  int z2 = v[2], z3 = v[6];
  int z1 = (z2 + z3) * F_0_541;
  int tmp2 = z1 + z3 * (-F_1_847);
  int tmp3 = z1 + z2 * F_0_765;
  z2 = v[0];
  z3 = v[4];
  int tmp0 = (z2 + z3) << CONST_BITS;
  int tmp1 = (z2 - z3) << CONST_BITS;
  const int tmp10 = tmp0 + tmp3, tmp13 = tmp0 - tmp3, tmp11 = tmp1 + tmp2, tmp12 = tmp1 - tmp2;
  tmp0 = v[7];
  tmp1 = v[5];
  tmp2 = v[3];
  tmp3 = v[1];
  z1 = tmp0 + tmp3;
  z2 = tmp1 + tmp2;
  z3 = tmp0 + tmp2;
  int z4 = tmp1 + tmp3;
  const int z5 = (z3 + z4) * F_1_175;
  tmp0 *= F_0_298;
  tmp1 *= F_2_053;
  tmp2 *= F_3_072;
  tmp3 *= F_1_501;
  z1 *= -F_0_899;
  z2 *= -F_2_562;
  z3 *= -F_1_961;
  z4 *= -F_0_390;
  z3 += z5;
  z4 += z5;
  tmp0 += z1 + z3;
  tmp1 += z2 + z4;
  tmp2 += z2 + z3;
  tmp3 += z1 + z4;
  const int r = 1 << (shift - 1);
  v[0] = (tmp10 + tmp3 + r) >> shift;
  v[7] = (tmp10 - tmp3 + r) >> shift;
  v[1] = (tmp11 + tmp2 + r) >> shift;
  v[6] = (tmp11 - tmp2 + r) >> shift;
  v[2] = (tmp12 + tmp1 + r) >> shift;
  v[5] = (tmp12 - tmp1 + r) >> shift;
  v[3] = (tmp13 + tmp0 + r) >> shift;
  v[4] = (tmp13 - tmp0 + r) >> shift;
}

constexpr int WS_BLOCK = 72;  // dwords per block in the LDS: 64 + 8, so that the eight blocks of a wave start on different banks

// grid (ceil(max blocks / 32), B), 256 threads: lane = 8 * (block of the wave) + (row, then column, then row of the block)
__global__ __launch_bounds__(256) void idct_kernel(const unsigned char* __restrict__ coefs, const JImg* __restrict__ imgs,
                                                 unsigned char* __restrict__ planes) {
  __shared__ __attribute__((aligned(16))) int ws[32 * WS_BLOCK];
  const JImg d = imgs[blockIdx.y];
  const int tid = threadIdx.x;
  const int g = blockIdx.x * 32 + (tid >> 3);  // block of the image, all components in one sequence
  const int r = tid & 7;
  const bool live = g < d.blocks;
  int* w = ws + (tid >> 3) * WS_BLOCK;
  const int c = !live ? 0 : (g < d.nb01[0] ? 0 : (g < d.nb01[1] ? 1 : 2));
  int v[8];
  if (live) {
    // row r of the block, dequantised: 16 bytes of coefficients x 16 bytes of the component's table
    const uint4 cv = *reinterpret_cast<const uint4*>(coefs + d.coef_off + jpegx::TABLE_BYTES + (size_t)g * 128 + r * 16);
    const uint4 qv = *reinterpret_cast<const uint4*>(coefs + d.coef_off + c * 128 + r * 16);
    const unsigned cw[4] = {cv.x, cv.y, cv.z, cv.w}, qw[4] = {qv.x, qv.y, qv.z, qv.w};
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      v[2 * j] = (int)(short)(cw[j] & 0xFFFFu) * (int)(qw[j] & 0xFFFFu);
      v[2 * j + 1] = ((int)cw[j] >> 16) * (int)(qw[j] >> 16);
    }
    *reinterpret_cast<int4*>(w + r * 8) = make_int4(v[0], v[1], v[2], v[3]);
    *reinterpret_cast<int4*>(w + r * 8 + 4) = make_int4(v[4], v[5], v[6], v[7]);
  }
  __syncthreads();
  if (live) {  // column r
#pragma unroll
    for (int k = 0; k < 8; ++k) v[k] = w[k * 8 + r];
    idct8(v, CONST_BITS - PASS1_BITS);
#pragma unroll
    for (int k = 0; k < 8; ++k) w[k * 8 + r] = v[k];
  }
  __syncthreads();
  if (live) {  // row r
    const int4 a = *reinterpret_cast<const int4*>(w + r * 8), b = *reinterpret_cast<const int4*>(w + r * 8 + 4);
    v[0] = a.x; v[1] = a.y; v[2] = a.z; v[3] = a.w;
    v[4] = b.x; v[5] = b.y; v[6] = b.z; v[7] = b.w;
    idct8(v, CONST_BITS + PASS1_BITS + 3);
    unsigned lo = 0, hi = 0;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      lo |= (unsigned)limit8(v[k] + 128) << (8 * k);
      hi |= (unsigned)limit8(v[k + 4] + 128) << (8 * k);
    }
    const int first = c == 0 ? 0 : (c == 1 ? d.nb01[0] : d.nb01[1]);  // (selects, not indexing: the descriptor stays in registers)
    const int bwc = c == 0 ? d.bw[0] : (c == 1 ? d.bw[1] : d.bw[2]);
    const int gc = g - first;  // block of the component's plane
    const int by = gc / bwc, bx = gc - by * bwc;
    const size_t plane = (size_t)d.plane_off + (size_t)first * 64;
    // (planes are whole blocks wide and start on multiples of 64 bytes: the 8-byte store is aligned)
    *reinterpret_cast<uint2*>(planes + plane + ((size_t)(by * 8 + r) * bwc + bx) * 8) = make_uint2(lo, hi);
  }
}

// chroma sample of pixel (x, y) from plane `p` (pitch in bytes), real extent cw x ch, as libjpeg's upsamplers give it
__device__ __forceinline__ int chroma_at(const unsigned char* __restrict__ p, int pitch, int cw, int ch, int hs, int vs, int x, int y) {
  if (hs == 1) return p[(size_t)y * pitch + x];
  const int cx = x >> 1;
  if (vs == 1) {
    const unsigned char* row = p + (size_t)y * pitch;
    const int a = row[cx];
    if (cw <= 2) return a;
    if (x & 1) return cx == cw - 1 ? a : (3 * a + row[cx + 1] + 2) >> 2;
    return cx == 0 ? a : (3 * a + row[cx - 1] + 1) >> 2;
  }
  const int cy = y >> 1;
  if (cw <= 2) return p[(size_t)cy * pitch + cx];
  const unsigned char* near = p + (size_t)cy * pitch;
  const unsigned char* far = p + (size_t)((y & 1) ? min(cy + 1, ch - 1) : max(cy - 1, 0)) * pitch;
  const int s = 3 * near[cx] + far[cx];
  if (x & 1) return cx == cw - 1 ? (4 * s + 7) >> 4 : (3 * s + 3 * near[cx + 1] + far[cx + 1] + 7) >> 4;
  return cx == 0 ? (4 * s + 8) >> 4 : (3 * s + 3 * near[cx - 1] + far[cx - 1] + 8) >> 4;
}

// grid (ceil(max items / 256), B): an item = four consecutive pixels of a row
__global__ __launch_bounds__(256) void rgb_kernel(const unsigned char* __restrict__ planes, const JImg* __restrict__ imgs,
                                                unsigned char* __restrict__ pixels) {
  const JImg d = imgs[blockIdx.y];
  const int per_row = (d.w + 3) >> 2;
  const long long item = (long long)blockIdx.x * 256 + threadIdx.x;
  if (item >= (long long)per_row * d.h) return;
  const int y = (int)(item / per_row), x0 = (int)(item - (long long)y * per_row) * 4;
  const int nx = min(4, d.w - x0);
  const unsigned char* py = planes + d.plane_off;
  const int ypitch = d.bw[0] * 8;
  // all four pixels are computed (past the right edge: the last column again) so that `out` stays in registers
  unsigned char out[12];
  if (d.ncomp == 1) {
#pragma unroll
    for (int i = 0; i < 4; ++i) out[3 * i] = out[3 * i + 1] = out[3 * i + 2] = py[(size_t)y * ypitch + min(x0 + i, d.w - 1)];
  } else {
    const unsigned char* pcb = py + (size_t)d.nb01[0] * 64;
    const unsigned char* pcr = py + (size_t)d.nb01[1] * 64;
    const int cpitch = d.bw[1] * 8;
    const int cw = (d.w + d.hs - 1) / d.hs, ch = (d.h + d.vs - 1) / d.vs;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int x = min(x0 + i, d.w - 1);
      const int Y = py[(size_t)y * ypitch + x];
      const int cb = chroma_at(pcb, cpitch, cw, ch, d.hs, d.vs, x, y) - 128;
      const int cr = chroma_at(pcr, cpitch, cw, ch, d.hs, d.vs, x, y) - 128;
      out[3 * i] = (unsigned char)limit8(Y + ((91881 * cr + 32768) >> 16));
      out[3 * i + 1] = (unsigned char)limit8(Y + ((-22554 * cb - 46802 * cr + 32768) >> 16));
      out[3 * i + 2] = (unsigned char)limit8(Y + ((116130 * cb + 32768) >> 16));
    }
  }
  unsigned char* o = pixels + d.pix_off + ((size_t)y * d.w + x0) * 3;
  if (nx == 4 && (reinterpret_cast<uintptr_t>(o) & 3) == 0) {
    unsigned* o4 = reinterpret_cast<unsigned*>(o);
#pragma unroll
    for (int j = 0; j < 3; ++j)
      o4[j] = (unsigned)out[4 * j] | ((unsigned)out[4 * j + 1] << 8) | ((unsigned)out[4 * j + 2] << 16) | ((unsigned)out[4 * j + 3] << 24);
  } else {
#pragma unroll
    for (int i = 0; i < 12; ++i)
      if (i < 3 * nx) o[i] = out[i];
  }
}

// image tables of at least 64 KiB, the plane scratch in the slot beside them; made once and never deleted (clipx_upload_ring.h)
clipx::UploadRing& table_ring() {
  static clipx::UploadRing* const ring = new clipx::UploadRing((size_t)64 << 10);
  return *ring;
}

}  // namespace

using clipx::fail;

extern "C" int clipx_jpeg_probe_host(const void* data, size_t n, int max_side, clipx_jpeg_desc* desc, size_t* record_bytes) {
  if (!desc || !record_bytes || max_side <= 0) return fail(CLIPX_E_ARG, "bad jpeg_probe arguments");
  jpegx::Desc d;
  if (jpegx::probe(data, n, max_side, &d) != jpegx::TAKEN) return CLIPX_JPEG_DEFERRED;
  memcpy(desc, &d, sizeof(d));
  *record_bytes = jpegx::record_bytes(d);
  return CLIPX_JPEG_TAKEN;
}

extern "C" int clipx_jpeg_entropy_host(const void* data, size_t n, int max_side, clipx_jpeg_desc* desc, void* record, size_t record_bytes) {
  if (!desc || !record || max_side <= 0) return fail(CLIPX_E_ARG, "bad jpeg_entropy arguments");
  jpegx::Desc d;
  if (jpegx::decode(data, n, max_side, &d, record, record_bytes) != jpegx::TAKEN) return CLIPX_JPEG_DEFERRED;
  memcpy(desc, &d, sizeof(d));
  return CLIPX_JPEG_TAKEN;
}

extern "C" int clipx_jpeg_pixels_device(int device, const void* coefs_dev, const clipx_jpeg_desc* descs, int B, void* pixels_dev,
                                        const int64_t* offsets, void* stream) {
  if (!coefs_dev || !descs || !pixels_dev || !offsets || B < 0) return fail(CLIPX_E_ARG, "bad jpeg_pixels arguments");
  if (B == 0) return CLIPX_OK;
  if (device < 0 || device >= 64 || B > 65535) return fail(CLIPX_E_ARG, "bad device or more than 65535 images");
  if (reinterpret_cast<uintptr_t>(coefs_dev) & 15) return fail(CLIPX_E_ARG, "the coefficient buffer must be 16-byte aligned");
  std::vector<JImg> tab((size_t)B);
  long long plane_bytes = 0, max_items = 1;
  int max_blocks = 1;
  for (int i = 0; i < B; ++i) {
    const clipx_jpeg_desc& s = descs[i];
    JImg& d = tab[i];
    // the descriptor is what the entropy stage wrote; anything else must not reach a kernel that indexes with it
    jpegx::Desc jd;
    memcpy(&jd, &s, sizeof(jd));
    long long mcus = 0;
    if (!jpegx::desc_consistent(jd, &mcus) || offsets[i] < 0)
      return fail(CLIPX_E_ARG, "jpeg descriptor " + std::to_string(i) + " is not one the entropy stage writes");
    d.coef_off = s.coef_off;
    d.plane_off = plane_bytes;
    d.pix_off = offsets[i];
    d.w = s.width; d.h = s.height; d.ncomp = s.ncomp; d.hs = s.hs; d.vs = s.vs;
    for (int c = 0; c < 3; ++c) { d.bw[c] = c < s.ncomp ? s.bw[c] : 0; d.bh[c] = c < s.ncomp ? s.bh[c] : 0; }
    d.blocks = s.blocks;
    d.nb01[0] = d.bw[0] * d.bh[0];
    d.nb01[1] = d.nb01[0] + d.bw[1] * d.bh[1];
    d.pad = 0;
    plane_bytes += (long long)s.blocks * 64;
    max_blocks = std::max(max_blocks, s.blocks);
    max_items = std::max(max_items, (long long)((s.width + 3) / 4) * s.height);
  }
  const size_t tab_bytes = tab.size() * sizeof(JImg);

  HIPCHK(hipSetDevice(device));
  hipStream_t st = (hipStream_t)stream;
  clipx::UploadRing& ring = table_ring();
  std::lock_guard<std::mutex> lk(ring.mu);
  clipx::UploadSlot* sl;
  if (int r = ring.take(device, tab_bytes, &sl)) return r;
  // the planes: at least 8 MiB, a growth takes a quarter more than was asked for
  if (sl->scratch.bytes < (size_t)plane_bytes)
    HIPCHK(sl->scratch.ensure(std::max((size_t)plane_bytes + (size_t)plane_bytes / 4, (size_t)8 << 20)));
  if (int r = ring.upload(sl, tab.data(), tab_bytes, st)) return r;
  const JImg* tab_dev = static_cast<const JImg*>((void*)sl->dev);
  unsigned char* planes = static_cast<unsigned char*>((void*)sl->scratch);
  hipLaunchKernelGGL(idct_kernel, dim3((max_blocks + 31) / 32, B), dim3(256), 0, st, (const unsigned char*)coefs_dev, tab_dev, planes);
  HIPCHK(hipGetLastError());
  hipLaunchKernelGGL(rgb_kernel, dim3((unsigned)((max_items + 255) / 256), B), dim3(256), 0, st, (const unsigned char*)planes, tab_dev,
                     (unsigned char*)pixels_dev);
  HIPCHK(hipGetLastError());
  return ring.commit(sl, st);
}
