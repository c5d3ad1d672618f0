// jpegx_entropy.h -- the entropy stage of the GPU JPEG decoder: marker parsing and Huffman decoding of ONE class of
// files into int16 DCT coefficients, on the host.  Plain C++: no device code, no HIP call, system headers only, so that
// tools/jpeg_entropy_check.cpp can drive it under the sanitizers and a decode process without a GPU can run it.
//
// The class ("taken"): SOF0 baseline, 8-bit samples, 8-bit quantisation tables, ONE scan interleaving all components (with or
// without DRI / RSTn), 1 component or 3 that libjpeg reads as YCbCr (a JFIF marker or component ids 1, 2, 3; no Adobe marker), luma
// sampling 1x1 / 2x1 / 2x2 with 1x1 chroma, both sides <= max_side.  Everything else -- and everything that does not parse
// CLEANLY (a bad Huffman code, a coefficient index past 63, an RSTn out of order, bytes between the entropy data and the next
// marker, a missing EOI, a truncated file) -- is "deferred": the caller decodes the file with Pillow, as it did before.  The rule
// is one-sided on purpose: a deferral costs time, a wrongly taken file would cost bytes.  Coefficients a legal 8-bit encoder cannot
// produce (|coefficient x quantiser| > 2047; a legal one stays below 1024 + q / 2) are deferred as well: libjpeg's C and SIMD
// inverse DCTs only agree on legal input, and the pixel stage restates neither's overflow behaviour.
//
// Output of decode(): a RECORD of record_bytes(desc) bytes
//   uint16 qt[3][64]      quantisation table of each component, NATURAL (row-major) order; unused components zero
//   int16  coef[blocks][64]  component 0's plane, then 1's, then 2's; the blocks of a plane in raster order of the plane padded
//                          to whole MCUs (bw[c] x bh[c] blocks); the 64 coefficients of a block in NATURAL order (index = 8 * row +
//                          column, the order the inverse DCT reads), DC prediction undone.
// Natural order everywhere: the zig-zag of the file is undone here, once.
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <string.h>
#include <memory>
#include <new>

namespace jpegx {

enum Status { DEFERRED = 0, TAKEN = 1 };

struct Desc {             // == clipx_jpeg_desc of include/clipx.h
  int32_t width, height;  // the image
  int32_t ncomp;          // 1 (grayscale) or 3 (YCbCr)
  int32_t hs, vs;         // luma sampling factors (1 or 2); chroma is 1 x 1; grayscale is 1 x 1 whatever the file declares
  int32_t bw[3], bh[3];   // blocks per row / column of each component's plane, padded to whole MCUs
  int32_t blocks;         // all planes together
  int32_t restart;        // MCUs per restart interval, 0 = none
  int32_t pad;
  int64_t coef_off;       // filled in by whoever packs records into one buffer: byte offset of this image's record (16-aligned)
};
static_assert(sizeof(Desc) == 64, "the descriptor is part of the C ABI");

constexpr size_t TABLE_BYTES = 3 * 64 * sizeof(uint16_t);
constexpr int MAX_ABS_DEQUANT = 2047;

inline size_t record_bytes(const Desc& d) { return TABLE_BYTES + (size_t)d.blocks * 64 * sizeof(int16_t); }

// Is `s` a descriptor the host stages write (probe / decode here, the scan preparation of jpegx_scan.h), with a coef_off a packer may
// have set?  The device stages index memory with these fields: anything else must not reach them.  True: *mcus = the image's MCUs.
// What only one stage reads (`restart`, the pixel offsets) is checked by that stage.
inline bool desc_consistent(const Desc& s, long long* mcus) {
  const bool gray = s.ncomp == 1;
  if (!(s.width >= 1 && s.height >= 1 && s.width <= 65535 && s.height <= 65535 && (gray || s.ncomp == 3) &&
        ((s.hs == 1 && s.vs == 1) || (!gray && s.hs == 2 && (s.vs == 1 || s.vs == 2))) && s.coef_off >= 0 && (s.coef_off & 15) == 0))
    return false;
  const int mx = (s.width + 8 * s.hs - 1) / (8 * s.hs), my = (s.height + 8 * s.vs - 1) / (8 * s.vs);
  const long long n = (long long)mx * my;
  bool ok = s.bw[0] == mx * s.hs && s.bh[0] == my * s.vs;
  for (int c = 1; c < s.ncomp; ++c) ok = ok && s.bw[c] == mx && s.bh[c] == my;
  if (!ok || n * (s.hs * s.vs + s.ncomp - 1) != s.blocks) return false;
  *mcus = n;
  return true;
}

namespace detail {

// natural (row-major) index of zig-zag position k
static const uint8_t NATURAL[64] = {0,  1,  8,  16, 9,  2,  3,  10, 17, 24, 32, 25, 18, 11, 4,  5,  12, 19, 26, 33, 40, 48,
                                    41, 34, 27, 20, 13, 6,  7,  14, 21, 28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23,
                                    30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63};

constexpr int LOOK = 9;

struct Huff {
  bool defined = false;
  int nvals = 0;
  uint16_t look[1 << LOOK];  // (length << 8) | symbol for codes of <= LOOK bits, 0 otherwise
  int16_t fast[1 << LOOK];   // AC tables: code AND value bits inside LOOK bits -> (value << 8) | (run << 4) | (bits used), else 0
  int32_t maxcode[17];       // largest code of each length, -1 where the length has none
  int32_t valoff[17];        // index of a length's first symbol minus its first code
  uint8_t vals[256];
};

inline bool build_huff(Huff& h, const uint8_t counts[16], const uint8_t* vals, int nvals) {
  h.defined = false;
  if (nvals > 256) return false;
  memset(h.look, 0, sizeof(h.look));
  memcpy(h.vals, vals, (size_t)nvals);
  h.nvals = nvals;
  int code = 0, k = 0;
  for (int len = 1; len <= 16; ++len) {
    const int c = counts[len - 1];
    h.valoff[len] = k - code;
    if (code + c > (1 << len)) return false;  // more codes than the length holds
    for (int i = 0; i < c; ++i, ++code, ++k) {
      if (len <= LOOK) {
        const int lo = code << (LOOK - len), n = 1 << (LOOK - len);
        for (int j = 0; j < n; ++j) h.look[lo + j] = (uint16_t)((len << 8) | vals[k]);
      }
    }
    h.maxcode[len] = c ? code - 1 : -1;
    code <<= 1;
  }
  h.defined = k == nvals;
  // a short code followed by a short value, decoded in one step (most coefficients of a photograph are +-1 .. +-7)
  for (int i = 0; i < (1 << LOOK); ++i) {
    h.fast[i] = 0;
    const unsigned e = h.look[i];
    const int len = (int)(e >> 8), run = (int)(e >> 4) & 15, mag = (int)e & 15;
    if (!e || !mag || len + mag > LOOK) continue;
    const int bits = (i >> (LOOK - len - mag)) & ((1 << mag) - 1);
    const int v = bits < (1 << (mag - 1)) ? bits - (1 << mag) + 1 : bits;
    if (v >= -128 && v <= 127) h.fast[i] = (int16_t)(v * 256 + run * 16 + len + mag);
  }
  return h.defined;
}

struct Frame {
  Desc d;
  int qsel[3] = {0, 0, 0}, id[3] = {0, 0, 0};
  bool have_sof = false, jfif = false;
  uint16_t qt[4][64];  // natural order
  bool qdef[4] = {false, false, false, false};
  Huff dc[4], ac[4];
  size_t scan = 0;  // offset of the first entropy-coded byte
  int dcsel[3] = {0, 0, 0}, acsel[3] = {0, 0, 0};
};

// Bit reader over the entropy-coded segment.  Stuffed FF 00 pairs are undone; at a marker (or the end of the input) it feeds zero
// bits and counts them in `fake`, and a decode that has consumed any of them (n < fake) has run past the data.
struct Bits {
  const uint8_t* p;
  const uint8_t* end;
  uint64_t acc = 0;
  int n = 0, fake = 0;
  // leaves more than 32 bits in `acc`: enough for a code (<= 16) and its value (<= 11)
  inline void fill() {
    if (n > 32) return;
    if (p + 4 <= end) {  // four bytes at once when none of them is 0xFF (no stuffing, no marker)
      const uint32_t w = ((uint32_t)p[0] << 24) | ((uint32_t)p[1] << 16) | ((uint32_t)p[2] << 8) | p[3];
      const uint32_t inv = ~w;
      if (!((inv - 0x01010101u) & ~inv & 0x80808080u)) {
        acc = (acc << 32) | w;
        n += 32;
        p += 4;
        return;
      }
    }
    while (n <= 56) {
      unsigned b;
      if (p < end && *p != 0xFF) {
        b = *p++;
      } else if (p + 1 < end && p[1] == 0) {  // (*p is 0xFF here)
        b = 0xFF;
        p += 2;
      } else {
        b = 0;
        fake += 8;
      }
      acc = (acc << 8) | b;
      n += 8;
    }
  }
  inline unsigned peek(int k) const { return (unsigned)((acc >> (n - k)) & ((1u << k) - 1)); }  // 1 <= k <= 16 <= n
  inline void skip(int k) { n -= k; }
  inline bool overrun() const { return n < fake; }
  // after the last MCU of an interval: at most 7 padding bits, then (fill bytes and) the marker `m`
  inline bool expect_marker(unsigned m) {
    const int real = n - fake;
    if (real < 0 || real >= 8) return false;
    if (p >= end || *p != 0xFF) return false;
    while (p + 1 < end && p[1] == 0xFF) ++p;
    if (p + 1 >= end || p[1] != m) return false;
    p += 2;
    acc = 0;
    n = fake = 0;
    return true;
  }
};

// one Huffman symbol, or -1
inline int symbol(Bits& b, const Huff& h) {
  const unsigned e = h.look[b.peek(LOOK)];
  if (e) {
    b.skip((int)(e >> 8));
    return (int)(e & 255);
  }
  for (int len = LOOK + 1; len <= 16; ++len) {
    const int c = (int)b.peek(len);
    if (c <= h.maxcode[len]) {
      const int idx = c + h.valoff[len];
      if (idx < 0 || idx >= h.nvals) return -1;
      b.skip(len);
      return h.vals[idx];
    }
  }
  return -1;
}

inline int extend(unsigned v, int s) { return v < (1u << (s - 1)) ? (int)v - (1 << s) + 1 : (int)v; }

inline bool decode_block(Bits& b, const Huff& dc, const Huff& ac, const uint16_t* q, int& pred, int16_t* out) {
  b.fill();
  int s = symbol(b, dc);
  if (s < 0 || s > 11) return false;
  int diff = 0;
  if (s) {
    diff = extend(b.peek(s), s);
    b.skip(s);
  }
  pred += diff;
  if (pred * (int)q[0] > MAX_ABS_DEQUANT || pred * (int)q[0] < -MAX_ABS_DEQUANT) return false;
  out[0] = (int16_t)pred;
  for (int k = 1; k < 64;) {
    b.fill();
    const int f = ac.fast[b.peek(LOOK)];
    if (f) {  // code and value in one look-up
      k += (f >> 4) & 15;
      if (k > 63) return false;
      b.skip(f & 15);
      const int nat = NATURAL[k], v = f >> 8;
      if (v * (int)q[nat] > MAX_ABS_DEQUANT || v * (int)q[nat] < -MAX_ABS_DEQUANT) return false;
      out[nat] = (int16_t)v;
      ++k;
      continue;
    }
    const int rs = symbol(b, ac);
    if (rs < 0) return false;
    const int r = rs >> 4;
    s = rs & 15;
    if (s == 0) {
      if (r != 15) {
        if (r != 0) return false;  // EOBn runs belong to progressive files
        break;
      }
      k += 16;
      if (k > 63) return false;  // a run of zeros that no coefficient can follow
      continue;
    }
    k += r;
    if (k > 63 || s > 10) return false;
    const int v = extend(b.peek(s), s);
    b.skip(s);
    const int nat = NATURAL[k];
    if (v * (int)q[nat] > MAX_ABS_DEQUANT || v * (int)q[nat] < -MAX_ABS_DEQUANT) return false;
    out[nat] = (int16_t)v;
    ++k;
  }
  return !b.overrun();
}

inline unsigned be16(const uint8_t* p) { return ((unsigned)p[0] << 8) | p[1]; }

// Markers up to the SOF (to_sos = false) or up to and including the SOS.  false = deferred.
inline bool parse(const uint8_t* data, size_t n, int max_side, bool to_sos, Frame& f) {
  if (!data || n < 4 || data[0] != 0xFF || data[1] != 0xD8) return false;
  size_t pos = 2;
  int restart = 0;
  for (;;) {
    if (pos + 4 > n || data[pos] != 0xFF) return false;  // (bytes before a marker: deferred)
    while (pos + 1 < n && data[pos + 1] == 0xFF) ++pos;  // fill bytes
    if (pos + 4 > n) return false;
    const unsigned m = data[pos + 1];
    const size_t len = be16(data + pos + 2);
    if (len < 2 || pos + 2 + len > n) return false;
    const uint8_t* seg = data + pos + 4;
    const size_t sl = len - 2;
    pos += 2 + len;
    if (m == 0xC0) {  // SOF0
      if (f.have_sof || sl < 6) return false;
      Desc& d = f.d;
      memset(&d, 0, sizeof(d));
      const int prec = seg[0], nc = seg[5];
      d.height = (int)be16(seg + 1);
      d.width = (int)be16(seg + 3);
      if (prec != 8 || (nc != 1 && nc != 3) || sl != (size_t)(6 + 3 * nc)) return false;
      if (d.width < 1 || d.height < 1 || d.width > max_side || d.height > max_side) return false;
      int hh[3], vv[3];
      for (int c = 0; c < nc; ++c) {
        f.id[c] = seg[6 + 3 * c];
        hh[c] = seg[7 + 3 * c] >> 4;
        vv[c] = seg[7 + 3 * c] & 15;
        f.qsel[c] = seg[8 + 3 * c];
        if (f.qsel[c] > 3 || hh[c] < 1 || hh[c] > 4 || vv[c] < 1 || vv[c] > 4) return false;
      }
      d.ncomp = nc;
      if (nc == 1) {
        d.hs = d.vs = 1;  // a single-component scan is not interleaved: one block per MCU whatever the factors say
      } else {
        if (!f.jfif && !(f.id[0] == 1 && f.id[1] == 2 && f.id[2] == 3)) return false;  // libjpeg would not (surely) say YCbCr
        if (hh[1] != 1 || vv[1] != 1 || hh[2] != 1 || vv[2] != 1) return false;
        if (!((hh[0] == 1 && vv[0] == 1) || (hh[0] == 2 && vv[0] == 1) || (hh[0] == 2 && vv[0] == 2))) return false;
        d.hs = hh[0];
        d.vs = vv[0];
      }
      const int mx = (d.width + 8 * d.hs - 1) / (8 * d.hs), my = (d.height + 8 * d.vs - 1) / (8 * d.vs);
      d.bw[0] = mx * d.hs;
      d.bh[0] = my * d.vs;
      d.blocks = d.bw[0] * d.bh[0];
      for (int c = 1; c < nc; ++c) {
        d.bw[c] = mx;
        d.bh[c] = my;
        d.blocks += mx * my;
      }
      f.have_sof = true;
      if (!to_sos) {
        d.restart = restart;
        return true;
      }
    } else if ((m >= 0xC1 && m <= 0xCF && m != 0xC4) || m == 0xDC || m == 0xD8 || m == 0xD9 || (m >= 0xD0 && m <= 0xD7) || m == 0x01 ||
               m == 0x00) {
      return false;  // other frame types (progressive, extended, lossless, arithmetic), DAC, DNL, stray SOI / EOI / RSTn / TEM
    } else if (m == 0xC4) {  // DHT: any number of tables
      size_t o = 0;
      while (o < sl) {
        if (o + 17 > sl) return false;
        const int tc = seg[o] >> 4, th = seg[o] & 15;
        int total = 0;
        for (int i = 0; i < 16; ++i) total += seg[o + 1 + i];
        if (tc > 1 || th > 3 || total > 256 || o + 17 + (size_t)total > sl) return false;
        if (!build_huff(tc ? f.ac[th] : f.dc[th], seg + o + 1, seg + o + 17, total)) return false;
        o += 17 + (size_t)total;
      }
    } else if (m == 0xDB) {  // DQT
      size_t o = 0;
      while (o < sl) {
        const int pq = seg[o] >> 4, tq = seg[o] & 15;
        if (pq != 0 || tq > 3 || o + 65 > sl) return false;  // (16-bit tables: deferred)
        for (int k = 0; k < 64; ++k) {
          if (seg[o + 1 + k] == 0) return false;  // (not a quantiser)
          f.qt[tq][NATURAL[k]] = seg[o + 1 + k];
        }
        f.qdef[tq] = true;
        o += 65;
      }
    } else if (m == 0xDD) {  // DRI
      if (sl != 2) return false;
      restart = (int)be16(seg);
    } else if (m == 0xE0) {
      if (sl >= 5 && memcmp(seg, "JFIF\0", 5) == 0) {
        if (f.have_sof) return false;  // (the colour space was decided at the SOF)
        f.jfif = true;
      }
    } else if (m == 0xEE) {
      if (sl >= 5 && memcmp(seg, "Adobe", 5) == 0) return false;  // Adobe transform flag: CMYK / YCCK / RGB files
    } else if (m == 0xDA) {  // SOS
      if (!f.have_sof) return false;
      const Desc& d = f.d;
      if (sl != (size_t)(4 + 2 * d.ncomp) || seg[0] != d.ncomp) return false;  // one scan with every component
      for (int c = 0; c < d.ncomp; ++c) {
        if (seg[1 + 2 * c] != f.id[c]) return false;
        f.dcsel[c] = seg[2 + 2 * c] >> 4;
        f.acsel[c] = seg[2 + 2 * c] & 15;
        if (f.dcsel[c] > 3 || f.acsel[c] > 3 || !f.dc[f.dcsel[c]].defined || !f.ac[f.acsel[c]].defined || !f.qdef[f.qsel[c]]) return false;
      }
      const uint8_t* t = seg + 1 + 2 * d.ncomp;
      if (t[0] != 0 || t[1] != 63 || t[2] != 0) return false;
      f.d.restart = restart;
      f.scan = pos;
      return true;
    }
    // APPn, COM and the rest carry nothing the decode needs
  }
}

}  // namespace detail

// Class and size of a file from its markers up to the SOF.  TAKEN: *d is filled in (coef_off = 0) and record_bytes(*d) is what
// decode() will write.  DEFERRED: nothing is written.
inline Status probe(const void* data, size_t n, int max_side, Desc* d) {
  std::unique_ptr<detail::Frame> f(new (std::nothrow) detail::Frame);
  if (!f || !detail::parse(static_cast<const uint8_t*>(data), n, max_side, false, *f)) return DEFERRED;
  *d = f->d;
  return TAKEN;
}

// The whole entropy stage.  TAKEN: *d and the record (record_bytes(*d) <= out_bytes) are written.  DEFERRED: neither `d` nor `out`
// is touched -- the coefficients are decoded into a buffer of the stage's own and copied out only when the file has parsed
// cleanly to its EOI.
inline Status decode(const void* data_, size_t n, int max_side, Desc* d, void* out, size_t out_bytes) {
  using namespace detail;
  const uint8_t* data = static_cast<const uint8_t*>(data_);
  std::unique_ptr<Frame> fp(new (std::nothrow) Frame);
  if (!fp || !parse(data, n, max_side, true, *fp)) return DEFERRED;
  Frame& f = *fp;
  const Desc& fd = f.d;
  const size_t need = record_bytes(fd);
  if (!out || out_bytes < need) return DEFERRED;
  const size_t ncoef = (size_t)fd.blocks * 64;
  std::unique_ptr<int16_t[]> coef(new (std::nothrow) int16_t[ncoef]());
  if (!coef) return DEFERRED;
  int16_t* plane[3] = {coef.get(), nullptr, nullptr};
  for (int c = 1; c < fd.ncomp; ++c) plane[c] = plane[c - 1] + (size_t)fd.bw[c - 1] * fd.bh[c - 1] * 64;
  const int hsc[3] = {fd.hs, 1, 1}, vsc[3] = {fd.vs, 1, 1};
  const int mx = fd.bw[0] / fd.hs, my = fd.bh[0] / fd.vs;
  Bits b;
  b.p = data + f.scan;
  b.end = data + n;
  int pred[3] = {0, 0, 0};
  long long left = fd.restart;  // MCUs until the next RSTn
  unsigned rst = 0;
  for (int y = 0; y < my; ++y) {
    for (int x = 0; x < mx; ++x) {
      if (fd.restart && left == 0) {
        if (!b.expect_marker(0xD0 + rst)) return DEFERRED;
        rst = (rst + 1) & 7;
        pred[0] = pred[1] = pred[2] = 0;
        left = fd.restart;
      }
      for (int c = 0; c < fd.ncomp; ++c) {
        const uint16_t* q = f.qt[f.qsel[c]];
        for (int v = 0; v < vsc[c]; ++v)
          for (int h = 0; h < hsc[c]; ++h) {
            const size_t blk = (size_t)(y * vsc[c] + v) * fd.bw[c] + (size_t)(x * hsc[c] + h);
            if (!decode_block(b, f.dc[f.dcsel[c]], f.ac[f.acsel[c]], q, pred[c], plane[c] + blk * 64)) return DEFERRED;
          }
      }
      --left;
    }
  }
  if (!b.expect_marker(0xD9)) return DEFERRED;  // EOI right behind the data: no second scan, nothing skipped
  *d = fd;
  uint16_t* qo = static_cast<uint16_t*>(out);
  memset(qo, 0, TABLE_BYTES);
  for (int c = 0; c < fd.ncomp; ++c) memcpy(qo + 64 * c, f.qt[f.qsel[c]], 64 * sizeof(uint16_t));
  memcpy(static_cast<uint8_t*>(out) + TABLE_BYTES, coef.get(), ncoef * sizeof(int16_t));
  return TAKEN;
}

}  // namespace jpegx
