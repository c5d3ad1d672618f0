// jpeg_split_kernels.hip -- the device side of the split Huffman decode: jpegx_split.h's runs with a workgroup's view
// of memory.  A translation unit of its own, so that huff_kernel (jpeg_huff_kernels.hip, which declares no LDS) compiles to the
// code it always had; HImg, WaveBytes and LaneSink come from jpeg_huff_dev.h, the host side stays in jpeg_huff_kernels.hip.
//
//   huff_split_kernel    one workgroup of 256 threads per (restart interval, image), the grid of huff_kernel.  An interval the cut
//                        leaves whole is not this kernel's: the workgroup leaves at once.  A split interval: the scan's tables, the
//                        quantisers and the zig-zag order are copied to the LDS, where the states of the at most 512 sub-sequences
//                        lie too (31.1 KiB in all); lane t owns sub-sequences t and t + 256.  Each lane reads the file through a
//                        dword it keeps (LaneBytes) and looks codes up in the LDS tables, per lane.  A round is decide /
//                        barrier-with-vote / decode / barrier; the tallies are scanned with wave shuffles and one hand-over
//                        through the LDS; the block rows are zeroed 16 bytes per lane; the write runs store int16s at their natural
//                        index and the smallest failure key is taken with one LDS atomic per failing run.  An interval that has
//                        not synchronised after max_rounds rounds is decoded by the workgroup's first wave exactly as huff_kernel
//                        decodes it (decode_interval + LaneSink); the other waves leave.
//   huff_unsplit_kernel  the same grid with one wave per (interval, image) and no LDS: huff_kernel's decode for the intervals the
//                        cut leaves whole, so that they keep huff_kernel's cost and occupancy; a split interval's wave leaves at
//                        once.  It also writes the record's tables and reports a record that fails the checks.
// Bounds: as in jpegx_split.h; rows are addressed from block indices below nmcu x blocks per MCU of the HOST descriptor only.

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "jpeg_huff_dev.h"
#include "jpegx_scan.h"
#include "jpegx_split.h"

namespace {

namespace P = jpegx::scan::split;

constexpr int SPLIT_THREADS = 256;
static_assert(P::MAX_SUB == 2 * SPLIT_THREADS, "two sub-sequences per lane");

// zig-zag position -> natural index (jpegx::detail::NATURAL, for the device)
__device__ const unsigned char NATURAL_OF[64] = {0,  1,  8,  16, 9,  2,  3,  10, 17, 24, 32, 25, 18, 11, 4,  5,  12, 19, 26, 33, 40, 48,
                                                 41, 34, 27, 20, 13, 6,  7,  14, 21, 28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23,
                                                 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63};

// The file's bytes as one lane reads them: the aligned dword it last loaded.  Nothing is loaded past `padded`.
struct LaneBytes {
  const unsigned char* file;  // 16-byte aligned
  unsigned padded;
  mutable unsigned at;  // offset of the dword held; ~0: none yet
  mutable unsigned w;
  __device__ __forceinline__ unsigned byte(unsigned pos) const {
    const unsigned a = pos & ~3u;
    if (a != at) {
      at = a;
      w = a + 4u <= padded ? *reinterpret_cast<const unsigned*>(file + a) : 0u;
    }
    return (w >> (8u * (pos & 3u))) & 255u;
  }
};

// The write pass's sink of one lane: int16 stores at the natural index, the range guard per coefficient.
struct LaneOut {
  short* coef;  // the image's coefficient area
  long long first1, first2;
  const unsigned short* qt;   // [3][64], in the LDS
  const unsigned char* nat;   // [64], in the LDS
  const unsigned short* q;
  short* row;
  __device__ __forceinline__ void begin(int c, long long blk) {
    q = qt + 64 * c;
    row = coef + ((c == 0 ? 0 : (c == 1 ? first1 : first2)) + blk) * 64;
  }
  __device__ __forceinline__ bool put(int k, int v) {
    const int n = nat[k & 63];
    row[n] = (short)v;
    const int t = (int)((unsigned)v * (unsigned)q[n]);
    return t <= jpegx::MAX_ABS_DEQUANT && t >= -jpegx::MAX_ABS_DEQUANT;
  }
};

// huff_kernel's decode of one interval by one wave (lane = threadIdx.x < 64)
__device__ __forceinline__ int serial_interval(const unsigned char* rec, const S::ScanHeader& h, const HImg& d, const S::Interval& I,
                                               const S::Geometry& g, unsigned short* out, int lane) {
  const unsigned short* qt = reinterpret_cast<const unsigned short*>(rec + S::QT_OFF);
  LaneSink sink;
  sink.q0 = qt[lane];
  sink.q1 = qt[64 + lane];
  sink.q2 = qt[128 + lane];
  sink.coef = reinterpret_cast<short*>(out + 192);
  sink.first1 = d.first[1];
  sink.first2 = d.first[2];
  sink.zz = ZIGZAG_OF[lane];
  sink.val = sink.q = 0;
  sink.row = sink.coef;
  WaveBytes src;
  src.file = rec + S::file_off(h.ntables, h.nintervals);
  src.padded = (h.file_bytes + 15u) & ~15u;
  src.lo = ~0u;
  src.w = 0;
  return S::decode_interval(src, g, reinterpret_cast<const S::HuffDev*>(rec + S::TAB_OFF), I.begin, I.end, I.first_mcu, I.nmcu, sink);
}

__device__ __forceinline__ unsigned wave_inclusive(unsigned v, int lane) {
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const unsigned n = __shfl_up(v, o);
    v += lane >= o ? n : 0u;
  }
  return v;
}

// grid (most intervals of an image, B), 256 threads
__global__ __launch_bounds__(SPLIT_THREADS) void huff_split_kernel(const unsigned char* __restrict__ scans, const HImg* __restrict__ imgs,
                                                                 unsigned char* __restrict__ coefs, int* __restrict__ status,
                                                                 int* __restrict__ rounds, unsigned split_bytes, int max_rounds) {
  __shared__ __attribute__((aligned(16))) S::HuffDev s_tab[6];
  __shared__ __attribute__((aligned(16))) P::Sub s_sub[P::MAX_SUB];
  __shared__ unsigned short s_qt[192];
  __shared__ unsigned char s_nat[64];
  __shared__ unsigned s_wave[4][4];
  __shared__ unsigned long long s_fail;

  const HImg d = imgs[blockIdx.y];
  const int iv = blockIdx.x, tid = threadIdx.x;
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
  if (code) return;  // (uniform over the workgroup: every thread read the same words; huff_unsplit_kernel reports it)
  unsigned short* out = reinterpret_cast<unsigned short*>(coefs + d.coef_off);
  const unsigned short* qt = reinterpret_cast<const unsigned short*>(rec + S::QT_OFF);
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
  const unsigned E = I.end - I.begin;
  const P::Cut cut = P::cut_of(E, split_bytes);
  if (cut.nsub == 0) return;  // huff_unsplit_kernel's
  int took = 0;  // the interval's rounds word
  bool serial = false;
  LaneBytes src;
  src.file = rec + S::file_off(h.ntables, h.nintervals);
  src.padded = (h.file_bytes + 15u) & ~15u;
  src.at = ~0u;
  src.w = 0;
  const int j0 = tid, j1 = tid + SPLIT_THREADS;

  {
    const unsigned* tw = reinterpret_cast<const unsigned*>(rec + S::TAB_OFF);
    unsigned* sw = reinterpret_cast<unsigned*>(s_tab);
    for (int i = tid; i < h.ntables * (int)(sizeof(S::HuffDev) / 4); i += SPLIT_THREADS) sw[i] = tw[i];
    if (tid < 192) s_qt[tid] = qt[tid];
    if (tid < 64) s_nat[tid] = NATURAL_OF[tid];
    if (tid == 0) s_fail = ~0ull;
    for (int j = tid; j < cut.nsub; j += SPLIT_THREADS) {
      s_sub[j].entry = j ? P::guess(src, I.begin, (unsigned)j * cut.s) : P::State{0, 0};
      s_sub[j].exit = P::State{0xFFFFFFFFu, 0xFFFFFFFFu};
    }
    __syncthreads();
    P::NoOut none;
    P::Fail nofail = {P::NO_KEY, S::CLEAN};
    bool fixed = false;
    int r = 1;
    for (; r <= max_rounds; ++r) {
      // the entries of a round come from the previous round's exits: every lane decides, the vote is the barrier, then they decode
      bool todo0 = r == 1 && j0 < cut.nsub, todo1 = r == 1 && j1 < cut.nsub;
      P::State want0 = {0, 0}, want1 = {0, 0};
      if (r > 1) {
        if (j0 >= 1 && j0 < cut.nsub) {
          want0 = s_sub[j0 - 1].exit;
          const P::State e = s_sub[j0].entry;
          todo0 = want0.pos != e.pos || want0.sk != e.sk;
        }
        if (j1 < cut.nsub) {
          want1 = s_sub[j1 - 1].exit;
          const P::State e = s_sub[j1].entry;
          todo1 = want1.pos != e.pos || want1.sk != e.sk;
        }
      }
      if (!__syncthreads_or(todo0 || todo1)) {
        fixed = true;
        break;
      }
      if (todo0) {
        if (r > 1) s_sub[j0].entry = want0;
        P::Tally t;
        const P::State x = P::run<false>(src, g, s_tab, I.begin, I.end, s_sub[j0].entry, P::limit_of(cut, j0, E), false, t, 0u, 0, none, nofail);
        s_sub[j0].exit = x;
        s_sub[j0].t = t;
      }
      if (todo1) {
        if (r > 1) s_sub[j1].entry = want1;
        P::Tally t;
        const P::State x = P::run<false>(src, g, s_tab, I.begin, I.end, s_sub[j1].entry, P::limit_of(cut, j1, E), false, t, 0u, 0, none, nofail);
        s_sub[j1].exit = x;
        s_sub[j1].t = t;
      }
      __syncthreads();
    }
    took = fixed ? r : -max_rounds;
    serial = !fixed;
  }

  if (serial) {  // it did not synchronise: huff_kernel's decode on the first wave
    if (tid >= 64) return;
    code = serial_interval(rec, h, d, I, g, out, tid);
    if (tid == 0) {
      if (code) atomicMax(status + blockIdx.y, code);
      if (rounds) atomicMax(reinterpret_cast<unsigned*>(rounds) + blockIdx.y, (unsigned)took);
    }
    return;
  }

  // exclusive scan of the tallies: lane t takes sub-sequences 2t and 2t + 1
  {
    const int lane = tid & 63, wave = tid >> 6;
    const int ja = 2 * tid, jb = 2 * tid + 1;
    P::Tally a = {0, {0, 0, 0}}, b = {0, {0, 0, 0}};
    if (ja < cut.nsub) a = s_sub[ja].t;
    if (jb < cut.nsub) b = s_sub[jb].t;
    unsigned v[4] = {a.blocks + b.blocks, a.dc[0] + b.dc[0], a.dc[1] + b.dc[1], a.dc[2] + b.dc[2]};
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      v[i] = wave_inclusive(v[i], lane);
      if (lane == 63) s_wave[i][wave] = v[i];
    }
    __syncthreads();  // (also: every tally has been read)
    unsigned ex[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      unsigned base = 0;
#pragma unroll
      for (int w = 0; w < 4; ++w) base += w < wave ? s_wave[i][w] : 0u;
      ex[i] = base + v[i];
    }
    ex[0] -= a.blocks + b.blocks;
    ex[1] -= a.dc[0] + b.dc[0];
    ex[2] -= a.dc[1] + b.dc[1];
    ex[3] -= a.dc[2] + b.dc[2];
    if (ja < cut.nsub) s_sub[ja].t = P::Tally{ex[0], {ex[1], ex[2], ex[3]}};
    if (jb < cut.nsub) s_sub[jb].t = P::Tally{ex[0] + a.blocks, {ex[1] + a.dc[0], ex[2] + a.dc[1], ex[3] + a.dc[2]}};
  }

  // the interval's block rows, zeroed 16 bytes per lane
  const int bpm = P::blocks_per_mcu(g);
  const unsigned nblocks = (unsigned)I.nmcu * (unsigned)bpm;
  short* coef = reinterpret_cast<short*>(out + 192);
  for (unsigned long long i = (unsigned)tid; i < 8ull * nblocks; i += SPLIT_THREADS) {
    const unsigned gb = (unsigned)(i >> 3);
    int c;
    long long blk;
    P::block_of(g, I.first_mcu + (int)(gb / (unsigned)bpm), (int)(gb % (unsigned)bpm), c, blk);
    short* row = coef + ((c == 0 ? 0 : (c == 1 ? d.first[1] : d.first[2])) + blk) * 64;
    reinterpret_cast<uint4*>(row)[i & 7] = make_uint4(0, 0, 0, 0);
  }
  __syncthreads();  // (rows zeroed, scanned tallies stored)

  LaneOut lo;
  lo.coef = coef;
  lo.first1 = d.first[1];
  lo.first2 = d.first[2];
  lo.qt = s_qt;
  lo.nat = s_nat;
  lo.q = s_qt;
  lo.row = coef;
  P::Fail fail = {P::NO_KEY, S::CLEAN};
  if (j0 < cut.nsub) {
    P::Tally t = s_sub[j0].t;
    P::run<true>(src, g, s_tab, I.begin, I.end, s_sub[j0].entry, P::limit_of(cut, j0, E), j0 == cut.nsub - 1, t, nblocks, I.first_mcu, lo, fail);
  }
  if (j1 < cut.nsub) {
    P::Tally t = s_sub[j1].t;
    P::run<true>(src, g, s_tab, I.begin, I.end, s_sub[j1].entry, P::limit_of(cut, j1, E), j1 == cut.nsub - 1, t, nblocks, I.first_mcu, lo, fail);
  }
  if (fail.key != P::NO_KEY) atomicMin(&s_fail, ((unsigned long long)fail.key << 32) | (unsigned)fail.code);
  __syncthreads();
  if (tid == 0) {
    const unsigned long long f = s_fail;
    if (f != ~0ull) atomicMax(status + blockIdx.y, (int)(unsigned)(f & 0xFFFFFFFFull));
    if (rounds) atomicMax(reinterpret_cast<unsigned*>(rounds) + blockIdx.y, (unsigned)took);
  }
}

// grid (most intervals of an image, B), 64 threads
__global__ __launch_bounds__(64) void huff_unsplit_kernel(const unsigned char* __restrict__ scans, const HImg* __restrict__ imgs,
                                                        unsigned char* __restrict__ coefs, int* __restrict__ status, unsigned split_bytes) {
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
    unsigned short* out = reinterpret_cast<unsigned short*>(coefs + d.coef_off);
    if (iv == 0) {  // the record's tables: the first interval's wave writes them
      const unsigned short* qt = reinterpret_cast<const unsigned short*>(rec + S::QT_OFF);
      out[lane] = qt[lane];
      out[64 + lane] = qt[64 + lane];
      out[128 + lane] = qt[128 + lane];
    }
    if (P::cut_of(I.end - I.begin, split_bytes).nsub != 0) return;  // huff_split_kernel's
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
    code = serial_interval(rec, h, d, I, g, out, lane);
  }
  if (code && lane == 0) atomicMax(status + blockIdx.y, code);
}

}  // namespace

hipError_t clipx_jpeg_launch_split(unsigned intervals, unsigned images, hipStream_t stream, const unsigned char* scans, const void* imgs,
                                   unsigned char* coefs, int* status, int* rounds, unsigned split_bytes, int max_rounds) {
  hipLaunchKernelGGL(huff_unsplit_kernel, dim3(intervals, images), dim3(64), 0, stream, scans, static_cast<const HImg*>(imgs), coefs, status,
                     split_bytes);
  const hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(huff_split_kernel, dim3(intervals, images), dim3(SPLIT_THREADS), 0, stream, scans, static_cast<const HImg*>(imgs), coefs,
                     status, rounds, split_bytes, max_rounds);
  return hipGetLastError();
}
