// jpegx_scan.h -- the Huffman stage of the GPU JPEG decoder, for the device (`gpu_huffman`).  Two things live here:
//
//   1. Host preparation (plain C++: no HIP call, system headers only).  A file of the accepted class is parsed to its SOS exactly as
//      jpegx_entropy.h parses it (its detail::parse, Huff and build_huff are reused), its entropy-coded bytes are walked for MARKERS
//      only -- no Huffman decoding -- and a SCAN RECORD is written: everything one wave per restart interval needs.
//   2. The interval decoder, written ONCE as templates usable from host and device (JPEGX_HD): bit reader, symbol look-up, block
//      loop and MCU loop with the semantics of jpegx_entropy.h's Bits / symbol / decode_block.  csrc/jpeg_huff_kernels.hip
//      instantiates it with a wave's byte window and a lane-per-coefficient sink; tools/jpeg_scan_check.cpp instantiates it with
//      plain memory under the sanitizers and compares verdict and record with jpegx::decode.
//
// The scan record (16-byte aligned, scan_bytes() long, all offsets relative to its start):
//   ScanHeader           64 bytes
//   uint16 qt[3][64]     quantisation table of each component, natural order; unused components zero
//   HuffDev tab[ntables] the DISTINCT Huffman tables the scan selects (header: dc_tab[c] / ac_tab[c] index them)
//   Interval ivl[nint]   first MCU, MCU count, first and one-past-last byte (file offsets) of each restart interval
//   uint8 file[n]        the file as it is (FF 00 is undone by the decoder; a late Pillow decode needs the whole file), padded to 16
//
// Equivalence with jpegx::decode (the argument in full: DESIGN 9).  The host stage decodes the intervals one after the other with a
// bit reader that stops at the first FF not followed by 00 and feeds counted zero bits there; it resets the predictors after an
// RSTn and requires, at every interval's end, 0 .. 7 unconsumed real bits, the reader AT the marker, (fill FFs and) the expected
// marker.  The marker walk finds the same stops and checks the same markers; an interval decoded on its own from its first byte
// with zero predictors sees the same bit string, so its blocks decode to the same symbols, and "clean" below restates the end
// condition.  Hence: decode() TAKEN <=> prepare() TAKEN and every interval clean, and the coefficients are the same.
#pragma once
#include "jpegx_entropy.h"

#if defined(__HIPCC__)
#define JPEGX_HD __host__ __device__
#else
#define JPEGX_HD
#endif

namespace jpegx {
namespace scan {

constexpr uint32_t MAGIC = 0x4e43534au;  // "JSCN"
constexpr int LOOK = detail::LOOK;

// interval / image status: 0 = clean, otherwise why not (the largest code of an image's intervals is reported)
enum Code : int32_t {
  CLEAN = 0,
  BAD_RECORD = 1,  // the record is not one prepare() writes for this descriptor (the decoder was not run)
  BAD_CODE = 2,    // no Huffman code matches, or a size category above 11 (DC) / 10 (AC)
  BAD_INDEX = 3,   // a coefficient index past 63
  BAD_EOB = 4,     // an EOBn run (progressive files)
  BAD_RANGE = 5,   // |coefficient x quantiser| > 2047
  OVERRUN = 6,     // a block consumed bits that were fed behind the interval's last byte
  TRAILING = 7,    // eight or more real bits are left behind the interval's last MCU
};

// a Huffman table in the form the device reads: dwords only, so that a wave-uniform look-up is one scalar load
struct HuffDev {
  uint32_t lf[1 << LOOK];  // low half: Huff::look, high half: Huff::fast
  int32_t maxcode[17];     // [0] unused (-1)
  int32_t valoff[17];      // [0] unused (0)
  int32_t nvals;
  int32_t pad;
  uint32_t vals[64];       // Huff::vals, four symbols to the dword, little end first
};
static_assert(sizeof(HuffDev) == 2448 && sizeof(HuffDev) % 16 == 0, "part of the scan record");

struct Interval {
  int32_t first_mcu, nmcu;
  uint32_t begin, end;  // entropy-coded bytes [begin, end) of the file; `end` is the FF of the marker that closes the interval
};
static_assert(sizeof(Interval) == 16, "part of the scan record");

struct ScanHeader {
  uint32_t magic;
  uint32_t total_bytes;  // of the record
  uint32_t file_bytes;
  int32_t nintervals;
  int32_t ntables;
  int32_t dc_tab[3], ac_tab[3];  // index of each component's tables in tab[]; unused components 0
  int32_t pad[5];
};
static_assert(sizeof(ScanHeader) == 64, "part of the scan record");

constexpr size_t QT_OFF = sizeof(ScanHeader);
constexpr size_t TAB_OFF = QT_OFF + TABLE_BYTES;
JPEGX_HD inline size_t ivl_off(int ntables) { return TAB_OFF + (size_t)ntables * sizeof(HuffDev); }
JPEGX_HD inline size_t file_off(int ntables, long long nintervals) { return ivl_off(ntables) + (size_t)nintervals * sizeof(Interval); }
JPEGX_HD inline size_t total_bytes(int ntables, long long nintervals, size_t file_bytes) {
  return (file_off(ntables, nintervals) + file_bytes + 15) & ~(size_t)15;
}
JPEGX_HD inline long long mcus_of(const Desc& d) { return (long long)(d.bw[0] / d.hs) * (d.bh[0] / d.vs); }
JPEGX_HD inline long long intervals_of(const Desc& d) {
  const long long m = mcus_of(d);
  return d.restart > 0 ? (m + d.restart - 1) / d.restart : 1;
}

// ---- the interval decoder, host and device ---------------------------------------------------------------------------------------

// What one interval's decode needs to know of the image.
struct Geometry {
  int ncomp, hs, vs;  // luma sampling (chroma 1 x 1)
  int mx;             // MCUs per row
  int bw[3];          // blocks per row of each component's plane
  int dc[3], ac[3];   // tables of each component (indices into tab[])
};

// Bit reader over bytes [p, end) of `src`.  FF 00 pairs are undone; behind the last byte zero bits are fed and counted in `fake`.
// Src: `unsigned byte(uint32_t pos)` for pos < end.
template <class Src>
struct Bits {
  Src src;
  uint32_t p, end;
  uint64_t acc;
  int n, fake;
  // leaves more than 56 bits: enough for a code (<= 16) and its value (<= 11)
  JPEGX_HD inline void fill() {
    while (n <= 56) {
      unsigned b = 0;
      if (p < end) b = src.byte(p);
      if (p < end && b != 0xFF) {
        ++p;
      } else if (p + 1 < end && src.byte(p + 1) == 0) {  // (byte p is 0xFF here)
        p += 2;
      } else {
        b = 0;
        fake += 8;
      }
      acc = (acc << 8) | b;
      n += 8;
    }
  }
  JPEGX_HD inline unsigned peek(int k) const { return (unsigned)((acc >> ((n - k) & 63)) & ((1u << k) - 1)); }  // 1 <= k <= 16 <= n
  JPEGX_HD inline void skip(int k) { n -= k; }
  JPEGX_HD inline bool overrun() const { return n < fake; }
};

// one Huffman symbol, or -1
template <class Src>
JPEGX_HD inline int symbol(Bits<Src>& b, const HuffDev& h) {
  const unsigned e = h.lf[b.peek(LOOK)] & 0xFFFFu;
  if (e) {
    b.skip((int)(e >> 8));
    return (int)(e & 255);
  }
  for (int len = LOOK + 1; len <= 16; ++len) {  // at most 7 probes
    const int c = (int)b.peek(len);
    if (c <= h.maxcode[len]) {
      const int idx = c + h.valoff[len];
      if (idx < 0 || idx >= h.nvals || idx > 255) return -1;
      b.skip(len);
      return (int)((h.vals[idx >> 2] >> (8 * (idx & 3))) & 255);
    }
  }
  return -1;
}

JPEGX_HD inline int extend(unsigned v, int s) { return v < (1u << (s - 1)) ? (int)v - (1 << s) + 1 : (int)v; }

// One block.  Sink: `bool put(int k, int v)` takes the coefficient at zig-zag position k (false: the range guard refused it),
// `bool end()` closes the block (false: the range guard refused one of its coefficients).  A sink may check at either place.
// Every pass of the loop advances k: at most 63 passes.
template <class Src, class Sink>
JPEGX_HD inline int decode_block(Bits<Src>& b, const HuffDev& dc, const HuffDev& ac, int& pred, Sink& sink) {
  b.fill();
  int s = symbol(b, dc);
  if (s < 0 || s > 11) return BAD_CODE;
  int diff = 0;
  if (s) {
    diff = extend(b.peek(s), s);
    b.skip(s);
  }
  pred += diff;
  if (!sink.put(0, pred)) return BAD_RANGE;
  for (int k = 1; k < 64;) {
    b.fill();
    const int f = (int)(int16_t)(ac.lf[b.peek(LOOK)] >> 16);
    if (f) {  // code and value in one look-up
      k += (f >> 4) & 15;
      if (k > 63) return BAD_INDEX;
      b.skip(f & 15);
      if (!sink.put(k, f >> 8)) return BAD_RANGE;
      ++k;
      continue;
    }
    const int rs = symbol(b, ac);
    if (rs < 0) return BAD_CODE;
    const int r = rs >> 4;
    s = rs & 15;
    if (s == 0) {
      if (r != 15) {
        if (r != 0) return BAD_EOB;  // EOBn runs belong to progressive files
        break;
      }
      k += 16;
      if (k > 63) return BAD_INDEX;  // a run of zeros that no coefficient can follow
      continue;
    }
    k += r;
    if (k > 63) return BAD_INDEX;
    if (s > 10) return BAD_CODE;
    const int v = extend(b.peek(s), s);
    b.skip(s);
    if (!sink.put(k, v)) return BAD_RANGE;
    ++k;
  }
  if (!sink.end()) return BAD_RANGE;
  return b.overrun() ? OVERRUN : CLEAN;
}

// the blocks of component C in MCU (x, y); Sink: `void begin(int c, long long blk)` opens block `blk` of component c's plane
template <int C, class Src, class Sink>
JPEGX_HD inline int decode_component(Bits<Src>& b, const Geometry& g, const HuffDev* tab, int x, int y, int& pred, Sink& sink) {
  const int nh = C ? 1 : g.hs, nv = C ? 1 : g.vs;
  for (int v = 0; v < nv; ++v)
    for (int h = 0; h < nh; ++h) {
      sink.begin(C, (long long)(y * nv + v) * g.bw[C] + (x * nh + h));
      const int st = decode_block(b, tab[g.dc[C]], tab[g.ac[C]], pred, sink);
      if (st) return st;
    }
  return CLEAN;
}

// One restart interval on its own: `nmcu` MCUs from MCU `first_mcu` on, predictors zero, bytes [begin, end).  Returns a Code.
// Clean: every block decoded, no fed bit consumed, fewer than 8 real bits left (unread bytes are real bits).
template <class Src, class Sink>
JPEGX_HD inline int decode_interval(const Src& src, const Geometry& g, const HuffDev* tab, uint32_t begin, uint32_t end, int first_mcu,
                                    int nmcu, Sink& sink) {
  Bits<Src> b{src, begin, end, 0, 0, 0};
  int p0 = 0, p1 = 0, p2 = 0;
  int y = first_mcu / g.mx, x = first_mcu - y * g.mx;
  for (int m = 0; m < nmcu; ++m) {
    int st = decode_component<0>(b, g, tab, x, y, p0, sink);
    if (st) return st;
    if (g.ncomp == 3) {
      st = decode_component<1>(b, g, tab, x, y, p1, sink);
      if (st) return st;
      st = decode_component<2>(b, g, tab, x, y, p2, sink);
      if (st) return st;
    }
    if (++x == g.mx) {
      x = 0;
      ++y;
    }
  }
  return (b.p != b.end || b.n - b.fake >= 8) ? TRAILING : CLEAN;
}

// Is `h` (a copy of a record's header) the header prepare() writes for a descriptor with `nintervals` (intervals_of) in a record of
// `avail` bytes?  When it is, every offset derived from it lies inside the record.
JPEGX_HD inline bool header_fits(const ScanHeader& h, long long nintervals, size_t avail) {
  if (h.magic != MAGIC || h.ntables < 1 || h.ntables > 6 || h.nintervals != nintervals) return false;
  if (total_bytes(h.ntables, h.nintervals, h.file_bytes) != h.total_bytes || h.total_bytes > avail) return false;
  for (int c = 0; c < 3; ++c)
    if (h.dc_tab[c] < 0 || h.dc_tab[c] >= h.ntables || h.ac_tab[c] < 0 || h.ac_tab[c] >= h.ntables) return false;
  return true;
}

// ---- host preparation ------------------------------------------------------------------------------------------------------------
namespace detail {

using jpegx::detail::Frame;
using jpegx::detail::Huff;

inline void to_dev(const Huff& h, HuffDev& o) {
  memset(&o, 0, sizeof(o));
  for (int i = 0; i < (1 << LOOK); ++i) o.lf[i] = (uint32_t)h.look[i] | ((uint32_t)(uint16_t)h.fast[i] << 16);
  o.maxcode[0] = -1;
  for (int len = 1; len <= 16; ++len) {
    o.maxcode[len] = h.maxcode[len];
    o.valoff[len] = h.valoff[len];
  }
  o.nvals = h.nvals;
  for (int i = 0; i < h.nvals; ++i) o.vals[i >> 2] |= (uint32_t)h.vals[i] << (8 * (i & 3));
}

// the distinct tables of the scan, DC tables first: sel[i] = (class << 2) | table id; fills the header's dc_tab / ac_tab
inline int select_tables(const Frame& f, ScanHeader& h, int sel[6]) {
  int nt = 0;
  for (int cls = 0; cls < 2; ++cls)
    for (int c = 0; c < f.d.ncomp; ++c) {
      const int want = (cls << 2) | (cls ? f.acsel[c] : f.dcsel[c]);
      int at = 0;
      while (at < nt && sel[at] != want) ++at;
      if (at == nt) sel[nt++] = want;
      (cls ? h.ac_tab : h.dc_tab)[c] = at;
    }
  return nt;
}

// Parse to the SOS and lay the record out.  false = deferred.
inline bool plan(const uint8_t* data, size_t n, int max_side, Frame& f, ScanHeader& h, int sel[6]) {
  if (n > 0xFFFFFFF0u - 16 || !jpegx::detail::parse(data, n, max_side, true, f)) return false;
  memset(&h, 0, sizeof(h));
  h.magic = MAGIC;
  h.file_bytes = (uint32_t)n;
  const long long nint = intervals_of(f.d);
  h.ntables = select_tables(f, h, sel);
  const size_t total = total_bytes(h.ntables, nint, n);
  if (nint > 0x7FFFFFFF || total > 0xFFFFFFF0u) return false;
  h.nintervals = (int32_t)nint;
  h.total_bytes = (uint32_t)total;
  return true;
}

}  // namespace detail

// Size of the scan record of a file whose markers up to the SOS put it in the class.  TAKEN: *d (coef_off = 0) and *bytes are
// written; prepare() may still defer the file (its marker walk).  DEFERRED: nothing is written.
inline Status probe(const void* data, size_t n, int max_side, Desc* d, size_t* bytes) {
  std::unique_ptr<detail::Frame> f(new (std::nothrow) detail::Frame);
  ScanHeader h;
  int sel[6];
  if (!f || !detail::plan(static_cast<const uint8_t*>(data), n, max_side, *f, h, sel)) return DEFERRED;
  *d = f->d;
  *bytes = h.total_bytes;
  return TAKEN;
}

// The scan record of a file.  TAKEN: *d and the record (probe()'s size <= out_bytes) are written.  DEFERRED: neither is touched --
// the marker walk runs before the first byte is written.
inline Status prepare(const void* data_, size_t n, int max_side, Desc* d, void* out, size_t out_bytes) {
  const uint8_t* data = static_cast<const uint8_t*>(data_);
  std::unique_ptr<detail::Frame> fp(new (std::nothrow) detail::Frame);
  ScanHeader h;
  int sel[6];
  if (!fp || !detail::plan(data, n, max_side, *fp, h, sel)) return DEFERRED;
  const detail::Frame& f = *fp;
  if (!out || out_bytes < h.total_bytes) return DEFERRED;
  std::unique_ptr<Interval[]> ivl(new (std::nothrow) Interval[(size_t)h.nintervals]);
  if (!ivl) return DEFERRED;
  // The marker walk.  An FF followed by anything but 00 (or by the end of the file) ends an interval; fill FFs in front of the
  // marker are skipped; interval i < last must end in RST(i mod 8), the last one in EOI.
  const long long mcus = mcus_of(f.d);
  const long long per = f.d.restart > 0 ? f.d.restart : mcus;
  size_t pos = f.scan;
  for (int i = 0; i < h.nintervals; ++i) {
    size_t j = pos;
    for (;;) {
      const void* hit = j < n ? memchr(data + j, 0xFF, n - j) : nullptr;
      if (!hit) return DEFERRED;  // the data runs to the end of the file: no EOI
      j = (size_t)(static_cast<const uint8_t*>(hit) - data);
      if (j + 1 >= n || data[j + 1] != 0) break;
      j += 2;
    }
    ivl[i].first_mcu = (int32_t)(i * per);
    ivl[i].nmcu = (int32_t)(mcus - i * per < per ? mcus - i * per : per);
    ivl[i].begin = (uint32_t)pos;
    ivl[i].end = (uint32_t)j;
    while (j + 1 < n && data[j + 1] == 0xFF) ++j;
    const unsigned want = i + 1 < h.nintervals ? 0xD0u + (unsigned)(i & 7) : 0xD9u;
    if (j + 1 >= n || data[j + 1] != want) return DEFERRED;
    pos = j + 2;
  }
  *d = f.d;
  uint8_t* o = static_cast<uint8_t*>(out);
  memset(o, 0, h.total_bytes);
  memcpy(o, &h, sizeof(h));
  for (int c = 0; c < f.d.ncomp; ++c) memcpy(o + QT_OFF + (size_t)c * 128, f.qt[f.qsel[c]], 128);
  for (int t = 0; t < h.ntables; ++t) {
    HuffDev hd;
    detail::to_dev((sel[t] & 4) ? f.ac[sel[t] & 3] : f.dc[sel[t] & 3], hd);
    memcpy(o + TAB_OFF + (size_t)t * sizeof(HuffDev), &hd, sizeof(hd));
  }
  memcpy(o + ivl_off(h.ntables), ivl.get(), (size_t)h.nintervals * sizeof(Interval));
  memcpy(o + file_off(h.ntables, h.nintervals), data, n);
  return TAKEN;
}

}  // namespace scan
}  // namespace jpegx
