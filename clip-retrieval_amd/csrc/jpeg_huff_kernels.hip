// jpeg_huff_kernels.hip -- the Huffman stage of the GPU JPEG decoder on the device (`gpu_huffman`): scan records
// (jpegx_scan.h: tables, restart-interval table, the file's bytes) -> the records clipx_jpeg_pixels_device reads, plus one status
// word per image.  The decoder itself is jpegx_scan.h's, the one tools/jpeg_scan_check.cpp runs under the sanitizers; this file
// gives it a wave's view of memory.
//
//   huff_kernel   one wave per restart interval, grid (most intervals of an image, B).  Huffman decoding is serial inside an
//                 interval, so the decode state -- bit buffer, byte position, zig-zag index, DC predictors -- is wave-uniform and
//                 every branch on it is a scalar branch.  The 64 lanes are the 64 NATURAL-order coefficients of the block under
//                 construction: a decoded value goes to the lane whose coefficient it is (one compare + select), and at the end of
//                 a block each lane stores its int16, one 128-byte row.  The range guard is one multiply and compare per lane
//                 against that lane's quantiser and a ballot.  The file's bytes are read 256 at a time, one dword per lane, and
//                 handed out with v_readlane; the tables are read through wave-uniform dword loads.  No LDS, no scratch.
// Bounds.  Everything that indexes the coefficient buffer comes from the HOST descriptor (checked as the pixel stage checks it);
// the device record is believed only as far as header_fits() and the interval's own check go, both against the extent the caller
// gave for the record.  A record that fails them ends in status BAD_RECORD without a decode.  Every loop is bounded: an interval
// decodes exactly its MCU count, a block at most 63 coefficient steps, a long code 7 probes, a refill 8 bytes.

#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string.h>
#include <algorithm>
#include <mutex>
#include <string>
#include <vector>

#include "../../include/clipx.h"
#include "clipx_host.h"
#include "jpegx_scan.h"

static_assert(sizeof(clipx_jpeg_desc) == sizeof(jpegx::Desc), "clipx_jpeg_desc is jpegx::Desc");

namespace {

namespace S = jpegx::scan;

struct HImg {            // one per image, in the table buffer
  long long scan_off;    // byte offset of the scan record in the scan buffer
  long long scan_avail;  // bytes the caller gave for it
  long long coef_off;    // byte offset of the output record in the coefficient buffer
  long long first[3];    // first block of each component's plane
  int ncomp, hs, vs, mx;
  int bw[3];
  int nint;              // restart intervals
  int mcus, per;         // MCUs of the image, MCUs per interval
};
static_assert(sizeof(HImg) % 8 == 0, "descriptors are read as an array");

// zig-zag position of natural index i: the inverse of jpegx::detail::NATURAL
__device__ const unsigned char ZIGZAG_OF[64] = {0,  1,  5,  6,  14, 15, 27, 28, 2,  4,  7,  13, 16, 26, 29, 42, 3,  8,  12, 17, 25, 30,
                                                41, 43, 9,  11, 18, 24, 31, 40, 44, 53, 10, 19, 23, 32, 39, 45, 52, 54, 20, 22, 33, 38,
                                                46, 51, 55, 60, 21, 34, 37, 47, 50, 56, 59, 61, 35, 36, 48, 49, 57, 58, 62, 63};

// The file's bytes as a wave reads them: a 256-byte window, one dword per lane, refilled when a position leaves it.  `padded` is the
// file's length rounded up to 16 -- still inside the record -- and nothing is loaded past it.
struct WaveBytes {
  const unsigned char* file;  // 16-byte aligned
  unsigned padded;
  unsigned lo;  // first byte of the window (a multiple of 256); ~0: none yet
  unsigned w;   // this lane's dword
  __device__ __forceinline__ unsigned byte(unsigned pos) {
    if ((pos & ~255u) != lo) {
      lo = pos & ~255u;
      const unsigned at = lo + 4u * threadIdx.x;
      w = at + 4u <= padded ? *reinterpret_cast<const unsigned*>(file + at) : 0u;
    }
    const unsigned d = (unsigned)__builtin_amdgcn_readlane((int)w, (int)((pos & 255u) >> 2));
    return (d >> (8u * (pos & 3u))) & 255u;
  }
};

// The block under construction, one coefficient per lane.
struct LaneSink {
  short* coef;  // the image's coefficient area
  long long first1, first2;
  int zz;       // zig-zag position of this lane's coefficient
  int q0, q1, q2;
  int val, q;
  short* row;
  __device__ __forceinline__ void begin(int c, long long blk) {
    val = 0;
    q = c == 0 ? q0 : (c == 1 ? q1 : q2);
    row = coef + ((c == 0 ? 0 : (c == 1 ? first1 : first2)) + blk) * 64;
  }
  __device__ __forceinline__ bool put(int k, int v) {
    val = zz == k ? v : val;
    return true;
  }
  __device__ __forceinline__ bool end() {
    row[threadIdx.x] = (short)val;
    const int t = val * q;
    return __ballot(t > jpegx::MAX_ABS_DEQUANT || t < -jpegx::MAX_ABS_DEQUANT) == 0ull;
  }
};

// grid (most intervals of an image, B), 64 threads
__global__ __launch_bounds__(64) void huff_kernel(const unsigned char* __restrict__ scans, const HImg* __restrict__ imgs,
                                                unsigned char* __restrict__ coefs, int* __restrict__ status) {
  const HImg d = imgs[blockIdx.y];
  const int iv = blockIdx.x, lane = threadIdx.x;
  if (iv >= d.nint) return;
  const unsigned char* rec = scans + d.scan_off;
  const S::ScanHeader h = *reinterpret_cast<const S::ScanHeader*>(rec);  // (the host made sure a header fits `scan_avail`)
  int code = S::header_fits(h, d.nint, (size_t)d.scan_avail) ? S::CLEAN : S::BAD_RECORD;
  S::Interval I = {0, 0, 0, 0};
  if (!code) {
    I = reinterpret_cast<const S::Interval*>(rec + S::ivl_off(h.ntables))[iv];
    const int first = iv * d.per;
    if (I.first_mcu != first || I.nmcu != min(d.per, d.mcus - first) || I.begin > I.end || I.end > h.file_bytes) code = S::BAD_RECORD;
  }
  if (!code) {
    const unsigned short* qt = reinterpret_cast<const unsigned short*>(rec + S::QT_OFF);
    unsigned short* out = reinterpret_cast<unsigned short*>(coefs + d.coef_off);
    LaneSink sink;
    sink.q0 = qt[lane];
    sink.q1 = qt[64 + lane];
    sink.q2 = qt[128 + lane];
    if (iv == 0) {  // the record's tables: the first interval's wave writes them
      out[lane] = (unsigned short)sink.q0;
      out[64 + lane] = (unsigned short)sink.q1;
      out[128 + lane] = (unsigned short)sink.q2;
    }
    sink.coef = reinterpret_cast<short*>(out + 192);
    sink.first1 = d.first[1];
    sink.first2 = d.first[2];
    sink.zz = ZIGZAG_OF[lane];
    sink.val = sink.q = 0;
    sink.row = sink.coef;
    S::Geometry g;
    g.ncomp = d.ncomp;
    g.hs = d.hs;
    g.vs = d.vs;
    g.mx = d.mx;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      g.bw[c] = d.bw[c];
      g.dc[c] = h.dc_tab[c];
      g.ac[c] = h.ac_tab[c];
    }
    WaveBytes src;
    src.file = rec + S::file_off(h.ntables, h.nintervals);
    src.padded = (h.file_bytes + 15u) & ~15u;
    src.lo = ~0u;
    src.w = 0;
    code = S::decode_interval(src, g, reinterpret_cast<const S::HuffDev*>(rec + S::TAB_OFF), I.begin, I.end, I.first_mcu, I.nmcu, sink);
  }
  if (code && lane == 0) atomicMax(status + blockIdx.y, code);
}

// per device: a small ring of image tables, each slot guarded by the event of the launch that last used it
struct Slot {
  void* tab_dev = nullptr;
  void* tab_host = nullptr;  // page-locked: the upload is a true asynchronous copy
  size_t tab_bytes = 0;
  hipEvent_t ev = nullptr;
  bool used = false;
};
struct Ring {
  Slot slot[4];
  int next = 0;
};
std::mutex g_mu;
Ring g_ring[64];

constexpr long long MAX_INTERVALS = 1ll << 22;  // of one image (8192 x 8192 at 4:4:4 with a restart marker behind every MCU has 2^20)
constexpr long long MAX_WAVES = 1ll << 24;      // of one launch

}  // namespace

using clipx::fail;

extern "C" int clipx_jpeg_scan_probe_host(const void* data, size_t n, int max_side, clipx_jpeg_desc* desc, size_t* scan_bytes) {
  if (!desc || !scan_bytes || max_side <= 0) return fail(CLIPX_E_ARG, "bad jpeg_scan_probe arguments");
  jpegx::Desc d;
  size_t bytes = 0;
  if (S::probe(data, n, max_side, &d, &bytes) != jpegx::TAKEN) return CLIPX_JPEG_DEFERRED;
  memcpy(desc, &d, sizeof(d));
  *scan_bytes = bytes;
  return CLIPX_JPEG_TAKEN;
}

extern "C" int clipx_jpeg_scan_host(const void* data, size_t n, int max_side, clipx_jpeg_desc* desc, void* scan, size_t scan_bytes) {
  if (!desc || !scan || max_side <= 0) return fail(CLIPX_E_ARG, "bad jpeg_scan arguments");
  jpegx::Desc d;
  if (S::prepare(data, n, max_side, &d, scan, scan_bytes) != jpegx::TAKEN) return CLIPX_JPEG_DEFERRED;
  memcpy(desc, &d, sizeof(d));
  return CLIPX_JPEG_TAKEN;
}

extern "C" int clipx_jpeg_entropy_device(int device, const void* scans_dev, const clipx_jpeg_desc* descs, const int64_t* scan_offs, int B,
                                         void* coefs_dev, int32_t* status_dev, void* stream) {
  if (!scans_dev || !descs || !scan_offs || !coefs_dev || !status_dev || B < 0) return fail(CLIPX_E_ARG, "bad jpeg_entropy_device arguments");
  if (B == 0) return CLIPX_OK;
  if (device < 0 || device >= 64 || B > 65535) return fail(CLIPX_E_ARG, "bad device or more than 65535 images");
  if ((reinterpret_cast<uintptr_t>(scans_dev) & 15) || (reinterpret_cast<uintptr_t>(coefs_dev) & 15))
    return fail(CLIPX_E_ARG, "the scan and coefficient buffers must be 16-byte aligned");
  std::vector<HImg> tab((size_t)B);
  long long max_int = 1;
  for (int i = 0; i < B; ++i) {
    const clipx_jpeg_desc& s = descs[i];
    HImg& d = tab[i];
    const bool gray = s.ncomp == 1;
    // the descriptor is what the host preparation wrote; anything else must not reach a kernel that indexes with it
    bool ok = s.width >= 1 && s.height >= 1 && s.width <= 65535 && s.height <= 65535 && (gray || s.ncomp == 3) &&
              ((s.hs == 1 && s.vs == 1) || (!gray && s.hs == 2 && (s.vs == 1 || s.vs == 2))) && s.coef_off >= 0 && (s.coef_off & 15) == 0 &&
              s.restart >= 0;
    long long mcus = 0;
    if (ok) {
      const int mx = (s.width + 8 * s.hs - 1) / (8 * s.hs), my = (s.height + 8 * s.vs - 1) / (8 * s.vs);
      mcus = (long long)mx * my;
      long long blocks = mcus * s.hs * s.vs;
      ok = s.bw[0] == mx * s.hs && s.bh[0] == my * s.vs;
      for (int c = 1; c < s.ncomp; ++c) {
        ok = ok && s.bw[c] == mx && s.bh[c] == my;
        blocks += mcus;
      }
      ok = ok && blocks == s.blocks;
    }
    if (!ok) return fail(CLIPX_E_ARG, "jpeg descriptor " + std::to_string(i) + " is not one the scan preparation writes");
    const long long per = s.restart > 0 ? std::min<long long>(s.restart, mcus) : mcus;
    const long long nint = (mcus + per - 1) / per;
    if (nint > MAX_INTERVALS) return fail(CLIPX_E_UNSUPPORTED, "image " + std::to_string(i) + " has more than 2^22 restart intervals");
    // record i lies in [scan_offs[i], scan_offs[i + 1]) and holds at least a header, the tables of one component and its intervals
    const long long off = scan_offs[i], avail = scan_offs[i + 1] - off;
    if (off < 0 || (off & 15) || avail < (long long)S::total_bytes(1, nint, 0))
      return fail(CLIPX_E_ARG, "scan record " + std::to_string(i) + ": bad offset or extent");
    d.scan_off = off;
    d.scan_avail = avail;
    d.coef_off = s.coef_off;
    d.first[0] = 0;
    d.first[1] = (long long)s.bw[0] * s.bh[0];
    d.first[2] = d.first[1] + (gray ? 0 : (long long)s.bw[1] * s.bh[1]);
    d.ncomp = s.ncomp; d.hs = s.hs; d.vs = s.vs; d.mx = s.bw[0] / s.hs;
    for (int c = 0; c < 3; ++c) d.bw[c] = c < s.ncomp ? s.bw[c] : 0;
    d.nint = (int)nint;
    d.mcus = (int)mcus;
    d.per = (int)per;
    max_int = std::max(max_int, nint);
  }
  const size_t tab_bytes = tab.size() * sizeof(HImg);

  HIPCHK(hipSetDevice(device));
  hipStream_t st = (hipStream_t)stream;
  std::lock_guard<std::mutex> lk(g_mu);
  Ring& r = g_ring[device];
  Slot* sl = &r.slot[r.next];
  r.next = (r.next + 1) & 3;
  if (sl->used) HIPCHK(hipEventSynchronize(sl->ev));  // the launch that last used this slot has finished
  if (!sl->ev) HIPCHK(hipEventCreateWithFlags(&sl->ev, hipEventDisableTiming));
  if (sl->tab_bytes < tab_bytes) {
    if (sl->tab_dev) (void)hipFree(sl->tab_dev);
    if (sl->tab_host) (void)hipHostFree(sl->tab_host);
    sl->tab_dev = sl->tab_host = nullptr;
    sl->tab_bytes = 0;
    const size_t want = std::max(tab_bytes, (size_t)64 << 10);
    HIPCHK(hipMalloc(&sl->tab_dev, want));
    HIPCHK(hipHostMalloc(&sl->tab_host, want, hipHostMallocDefault));
    sl->tab_bytes = want;
  }
  memcpy(sl->tab_host, tab.data(), tab_bytes);
  HIPCHK(hipMemcpyAsync(sl->tab_dev, sl->tab_host, tab_bytes, hipMemcpyHostToDevice, st));
  HIPCHK(hipMemsetAsync(status_dev, 0, (size_t)B * sizeof(int32_t), st));
  // (images per launch: a batch of files with a restart marker behind every MCU must not outgrow a grid)
  const int step = (int)std::max<long long>(1, std::min<long long>(B, MAX_WAVES / max_int));
  for (int b0 = 0; b0 < B; b0 += step) {
    const int nb = std::min(step, B - b0);
    hipLaunchKernelGGL(huff_kernel, dim3((unsigned)max_int, (unsigned)nb), dim3(64), 0, st, (const unsigned char*)scans_dev,
                       (const HImg*)sl->tab_dev + b0, (unsigned char*)coefs_dev, (int*)status_dev + b0);
    HIPCHK(hipGetLastError());
  }
  HIPCHK(hipEventRecord(sl->ev, st));
  sl->used = true;
  return CLIPX_OK;
}
