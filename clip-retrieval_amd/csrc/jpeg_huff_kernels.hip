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
#include "clipx_upload_ring.h"
#include "jpegx_scan.h"
#include "jpegx_split.h"
#include "jpeg_huff_dev.h"  // HImg, WaveBytes, LaneSink: shared with jpeg_split_kernels.hip

static_assert(sizeof(clipx_jpeg_desc) == sizeof(jpegx::Desc), "clipx_jpeg_desc is jpegx::Desc");

namespace {

namespace P = jpegx::scan::split;

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

// image tables of at least 64 KiB; made once and never deleted (clipx_upload_ring.h)
clipx::UploadRing& table_ring() {
  static clipx::UploadRing* const ring = new clipx::UploadRing((size_t)64 << 10);
  return *ring;
}

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

// split_bytes 0: huff_kernel over the whole batch, as ever.  Otherwise the batch is cut into runs of consecutive images: a run of
// images whose record extent leaves no room for an interval of 2 x split_bytes goes to huff_kernel; every other run gets two
// launches on the same grid, huff_unsplit_kernel for the intervals the cut leaves whole (the host cannot see an interval's length:
// it lies in the device record) and huff_split_kernel for the others.  They write disjoint rows.
static int entropy_launch(int device, const void* scans_dev, const clipx_jpeg_desc* descs, const int64_t* scan_offs, int B, void* coefs_dev,
                          int32_t* status_dev, unsigned split_bytes, int max_rounds, int32_t* rounds_dev, void* stream) {
  if (!scans_dev || !descs || !scan_offs || !coefs_dev || !status_dev || B < 0) return fail(CLIPX_E_ARG, "bad jpeg_entropy_device arguments");
  if (B == 0) return CLIPX_OK;
  if (device < 0 || device >= 64 || B > 65535) return fail(CLIPX_E_ARG, "bad device or more than 65535 images");
  if ((reinterpret_cast<uintptr_t>(scans_dev) & 15) || (reinterpret_cast<uintptr_t>(coefs_dev) & 15))
    return fail(CLIPX_E_ARG, "the scan and coefficient buffers must be 16-byte aligned");
  std::vector<HImg> tab((size_t)B);
  std::vector<char> may_split((size_t)B, 0);
  for (int i = 0; i < B; ++i) {
    const clipx_jpeg_desc& s = descs[i];
    HImg& d = tab[i];
    const bool gray = s.ncomp == 1;
    // the descriptor is what the host preparation wrote; anything else must not reach a decoder that indexes with it
    jpegx::Desc jd;
    memcpy(&jd, &s, sizeof(jd));
    long long mcus = 0;
    if (!jpegx::desc_consistent(jd, &mcus) || s.restart < 0)
      return fail(CLIPX_E_ARG, "jpeg descriptor " + std::to_string(i) + " is not one the scan preparation writes");
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
    // (the record holds header, at least a DC and an AC table, intervals and the file: an interval cannot be longer than what is
    // left for the file)
    may_split[i] = split_bytes && avail - (long long)S::total_bytes(2, nint, 0) >= 2ll * split_bytes;
  }
  const size_t tab_bytes = tab.size() * sizeof(HImg);

  HIPCHK(hipSetDevice(device));
  hipStream_t st = (hipStream_t)stream;
  clipx::UploadRing& ring = table_ring();
  std::lock_guard<std::mutex> lk(ring.mu);
  clipx::UploadSlot* sl;
  if (int r = ring.take(device, tab_bytes, &sl)) return r;
  if (int r = ring.upload(sl, tab.data(), tab_bytes, st)) return r;
  const HImg* tab_dev = static_cast<const HImg*>((void*)sl->dev);
  HIPCHK(hipMemsetAsync(status_dev, 0, (size_t)B * sizeof(int32_t), st));
  if (rounds_dev) HIPCHK(hipMemsetAsync(rounds_dev, 0, (size_t)B * sizeof(int32_t), st));
  for (int r0 = 0; r0 < B;) {
    int r1 = r0 + 1;
    long long max_int = tab[r0].nint;
    while (r1 < B && may_split[r1] == may_split[r0]) max_int = std::max<long long>(max_int, tab[r1++].nint);
    // (images per launch: a batch of files with a restart marker behind every MCU must not outgrow a grid)
    const int step = (int)std::max<long long>(1, std::min<long long>(r1 - r0, MAX_WAVES / max_int));
    for (int b0 = r0; b0 < r1; b0 += step) {
      const int nb = std::min(step, r1 - b0);
      if (may_split[r0]) {
        HIPCHK(clipx_jpeg_launch_split((unsigned)max_int, (unsigned)nb, st, (const unsigned char*)scans_dev, tab_dev + b0,
                                       (unsigned char*)coefs_dev, (int*)status_dev + b0, rounds_dev ? (int*)rounds_dev + b0 : (int*)nullptr,
                                       split_bytes, max_rounds));
      } else {
        hipLaunchKernelGGL(huff_kernel, dim3((unsigned)max_int, (unsigned)nb), dim3(64), 0, st, (const unsigned char*)scans_dev,
                           tab_dev + b0, (unsigned char*)coefs_dev, (int*)status_dev + b0);
      }
      HIPCHK(hipGetLastError());
    }
    r0 = r1;
  }
  return ring.commit(sl, st);
}

extern "C" int clipx_jpeg_entropy_device(int device, const void* scans_dev, const clipx_jpeg_desc* descs, const int64_t* scan_offs, int B,
                                         void* coefs_dev, int32_t* status_dev, void* stream) {
  return entropy_launch(device, scans_dev, descs, scan_offs, B, coefs_dev, status_dev, 0, 0, nullptr, stream);
}

static bool split_ok(const clipx_jpeg_split* split) {
  return split && P::valid_split_bytes(split->split_bytes) && split->max_rounds >= 0 && split->reserved[0] == 0 && split->reserved[1] == 0;
}

extern "C" int clipx_jpeg_entropy_split_device(int device, const void* scans_dev, const clipx_jpeg_desc* descs, const int64_t* scan_offs,
                                               int B, void* coefs_dev, int32_t* status_dev, const clipx_jpeg_split* split,
                                               int32_t* rounds_dev, void* stream) {
  if (!split_ok(split)) return fail(CLIPX_E_ARG, "jpeg split: split_bytes must be 0 or a power of two 32 .. 1024, max_rounds >= 0, reserved 0");
  return entropy_launch(device, scans_dev, descs, scan_offs, B, coefs_dev, status_dev, (unsigned)split->split_bytes,
                        split->max_rounds ? split->max_rounds : P::DEFAULT_MAX_ROUNDS, rounds_dev, stream);
}

extern "C" int clipx_jpeg_entropy_split_host(const void* scan, size_t scan_bytes, const clipx_jpeg_desc* desc, const clipx_jpeg_split* split,
                                             void* record, size_t record_bytes, int32_t* status, int32_t* rounds) {
  if (!scan || !desc || !record || !status || !rounds) return fail(CLIPX_E_ARG, "bad jpeg_entropy_split_host arguments");
  if (!split_ok(split)) return fail(CLIPX_E_ARG, "jpeg split: split_bytes must be 0 or a power of two 32 .. 1024, max_rounds >= 0, reserved 0");
  jpegx::Desc d;
  memcpy(&d, desc, sizeof(d));
  long long mcus = 0;
  if (!jpegx::desc_consistent(d, &mcus) || d.restart < 0 || S::intervals_of(d) > MAX_INTERVALS) return fail(CLIPX_E_ARG, "the jpeg descriptor is not one the scan preparation writes");
  if (record_bytes < jpegx::record_bytes(d)) return fail(CLIPX_E_ARG, "the record buffer is smaller than the descriptor's record");
  if ((reinterpret_cast<uintptr_t>(scan) & 15) || scan_bytes < S::total_bytes(1, S::intervals_of(d), 0)) return fail(CLIPX_E_ARG, "the scan record is not 16-byte aligned or shorter than its fixed part");
  P::decode_record_host(static_cast<const uint8_t*>(scan), scan_bytes, d, (uint32_t)split->split_bytes,
                        split->max_rounds ? split->max_rounds : P::DEFAULT_MAX_ROUNDS, static_cast<uint8_t*>(record), status, rounds);
  return CLIPX_OK;
}
