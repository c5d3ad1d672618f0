// jpeg_huff_dev.h -- what the kernels of the Huffman stage share (jpeg_huff_kernels.hip: huff_kernel; jpeg_split_kernels.hip: the split
// decode of DESIGN 9.2): the per-image table entry and a wave's view of the file and of the block under construction.  Each
// translation unit has its own copy of these types (unnamed namespace); the table crosses between them as bytes.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "jpegx_scan.h"

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

}  // namespace

// jpeg_split_kernels.hip: huff_unsplit_kernel, then huff_split_kernel, over grid (intervals, images) on `stream`; imgs: HImg[images]
hipError_t clipx_jpeg_launch_split(unsigned intervals, unsigned images, hipStream_t stream, const unsigned char* scans, const void* imgs,
                                   unsigned char* coefs, int* status, int* rounds, unsigned split_bytes, int max_rounds);
