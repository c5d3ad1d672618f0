// jpegx_split.h -- self-synchronising Huffman decode INSIDE a restart interval (`huffman_split`), written once for host
// and device (JPEGX_HD, no HIP call, system headers only through jpegx_scan.h).  csrc/jpeg_split_kernels.hip gives it a workgroup's
// view of memory; tools/jpeg_split_check.cpp and clipx_jpeg_entropy_split_host run it with the lanes as a loop.
//
// The cut.  An interval of E = end - begin entropy-coded bytes (as they lie in the file) is split when split_bytes != 0 and
// 2 * split_bytes <= E < MAX_SPLIT_BYTES; every other interval takes jpegx_scan.h's serial decode_interval, untouched.  The
// sub-sequence size s is split_bytes doubled until the interval has at most MAX_SUB = 512 sub-sequences (32 bytes of state each:
// 16 KiB of LDS next to the scan's tables, at most 6 x 2448 bytes); sub-sequence j covers bytes [j s, min((j + 1) s, E)) of the
// interval.  MAX_SPLIT_BYTES = 2^26 keeps every bit position and every key (4 x block + phase) below 2^31.
//
// The state at a symbol boundary: bit position in the stuffed stream relative to `begin` (normalised: never on the 00 of an FF 00
// pair, and clamped to 8 E with the FED flag once zero bits behind `end` have been reached), block slot inside the MCU, zig-zag
// index k (0: a DC symbol is next).  Two decoders in the same state decode alike from there on, up to the DC predictors.
//
// Rounds (Jacobi): in round 1 sub-sequence 0 starts from the true state and every other one from a guess (its first bit, slot 0,
// k 0); each decodes symbols until the first boundary at or past its last bit and stores that exit, the blocks that ended inside
// it and the sum of the DC differences per component.  In round r > 1 every sub-sequence whose predecessor's stored exit differs
// from the entry it last used decodes again from that exit.  A round in which nothing decodes is the fixed point, and the fixed
// point is the serial decode (sub-sequence 0 is true; j is true once j - 1 is true and j has decoded from its exit): at most nsub
// + 1 rounds.  Speculative runs never stop at an impossible symbol: they skip one bit, end the block and go on with the next slot,
// a fixed rule, so that the decode from a state stays a function of the state.
//
// Write pass.  Exclusive scans over the tallies give each sub-sequence its first block and its entry predictors; the interval's
// block rows are zeroed; one more run per sub-sequence stores coefficients at their natural index and finds the failures.  The
// verdict is the smallest key 4 x block + phase over all runs, phase 0: BAD_CODE / BAD_INDEX / BAD_EOB at a symbol, 1: BAD_RANGE
// (judged at the block's end, as the device sink of huff_kernel judges it), 2: OVERRUN at the block's end, 3: TRAILING behind the
// last block -- the order in which decode_interval meets them; no key, CLEAN.  Everything in front of the first failure is the
// serial decode, so that key is decode_interval's verdict; what lies behind it is never looked at (keys only compare smaller).
//
// Bounds.  A run makes at least one bit of progress per step (a code has at least one bit, the recovery skips one) and stops at its
// limit, which is at most 8 E; the last sub-sequence's write run may go on behind 8 E only until the block in progress, or one
// more, has ended (a block ends after at most 64 steps).  Rounds are at most max_rounds, the write pass stops at the block count
// nmcu x blocks per MCU of the HOST descriptor, table indices are masked or checked as in jpegx_scan.h, and every byte is read
// through Bits<Src>, which reads nothing outside [begin, end).
#pragma once
#include "jpegx_scan.h"

namespace jpegx {
namespace scan {
namespace split {

constexpr int MAX_SUB = 512;
constexpr uint32_t MAX_SPLIT_BYTES = 1u << 26;
constexpr int DEFAULT_MAX_ROUNDS = 16;  // the bench files need at most 13 rounds at 128 bytes
constexpr uint32_t FED = 1u << 16;
constexpr uint32_t NO_KEY = 0xFFFFFFFFu;
constexpr int NOT_SYNCHRONISED = -1;  // decode_split(): the cap was reached, decode serially

JPEGX_HD inline bool valid_split_bytes(int v) { return v == 0 || (v >= 32 && v <= 1024 && (v & (v - 1)) == 0); }

struct Cut {
  uint32_t s;  // bytes per sub-sequence
  int nsub;    // 0: the interval is not split
};
JPEGX_HD inline Cut cut_of(uint32_t E, uint32_t split_bytes) {
  Cut c = {0, 0};
  if (split_bytes == 0 || E < 2 * split_bytes || E >= MAX_SPLIT_BYTES) return c;
  uint32_t s = split_bytes;
  while ((E + s - 1) / s > (uint32_t)MAX_SUB) s *= 2;
  c.s = s;
  c.nsub = (int)((E + s - 1) / s);
  return c;
}

struct State {
  uint32_t pos;  // bit position relative to `begin`
  uint32_t sk;   // k | slot << 8 | FED
};
struct Tally {
  uint32_t blocks;  // block ends inside the sub-sequence; after the scan: blocks in front of it
  uint32_t dc[3];   // sum of the DC differences per component (wrapping); after the scan: the entry predictors
};
struct Sub {
  State entry, exit;
  Tally t;
};
static_assert(sizeof(Sub) == 32, "MAX_SUB of them lie in the LDS");
struct Fail {
  uint32_t key;  // 4 x block + phase, NO_KEY: none
  int32_t code;
};
JPEGX_HD inline void note(Fail& f, uint32_t block, uint32_t phase, int code) {
  const uint32_t key = 4u * block + phase;
  if (key < f.key) {
    f.key = key;
    f.code = code;
  }
}

JPEGX_HD inline int blocks_per_mcu(const Geometry& g) { return g.ncomp == 3 ? g.hs * g.vs + 2 : 1; }

// the plane and the block inside it of block `slot` of MCU `mcu`
JPEGX_HD inline void block_of(const Geometry& g, int mcu, int slot, int& c, long long& blk) {
  const int nl = g.ncomp == 3 ? g.hs * g.vs : 1;
  const int y = mcu / g.mx, x = mcu - y * g.mx;
  if (slot < nl) {
    const int v = slot / g.hs, h = slot - v * g.hs;
    c = 0;
    blk = (long long)(y * (nl / g.hs) + v) * g.bw[0] + (x * g.hs + h);
  } else {
    c = slot - nl + 1;
    blk = (long long)y * (c == 1 ? g.bw[1] : g.bw[2]) + x;
  }
}

// bit position of the reader's next bit relative to `begin`: the fill pointer less what the unread bytes of the accumulator cost in
// the file (an FF costs two bytes, fed zero bytes one each)
template <class Src>
JPEGX_HD inline uint32_t position(const Bits<Src>& b, uint32_t begin) {
  const int nb = (b.n + 7) >> 3;
  const uint64_t m = nb >= 8 ? ~0ull : ((1ull << (8 * nb)) - 1);
  const uint64_t t = ~b.acc & m;  // a zero byte: an FF among the unread bytes, or a byte above them
  const uint64_t nz = (((t & 0x7f7f7f7f7f7f7f7full) + 0x7f7f7f7f7f7f7f7full) | t) & 0x8080808080808080ull;
  const int ff = (8 - (int)__builtin_popcountll(nz)) - (8 - nb);
  return 8u * ((b.p - begin) + (uint32_t)(b.fake >> 3) - (uint32_t)(nb + ff)) + (uint32_t)(8 * nb - b.n);
}

// the guess sub-sequence j starts from in round 1
template <class Src>
JPEGX_HD inline State guess(const Src& src, uint32_t begin, uint32_t at) {
  State st = {8u * at, 0};
  if (at > 0 && src.byte(begin + at - 1) == 0xFF) st.pos += 8;  // the 00 of an FF 00 pair
  return st;
}

// One run of a sub-sequence from `in` to the first symbol boundary at or past bit `limit` (<= 8 E).
//   WRITE false: a speculative run.  t receives the tally, nothing else is written.
//   WRITE true:  t holds the blocks in front of the run and the entry predictors; coefficients go to `out` (`void begin(int c, long
//                long blk)`, `bool put(int k, int v)`: false when the range guard refuses it) for blocks below `nblocks`, where the
//                run stops; failures are noted in `fail`.  `last`: the run goes on behind the limit until a block has ended there.
template <bool WRITE, class Src, class Out>
JPEGX_HD inline State run(const Src& src, const Geometry& g, const HuffDev* tab, uint32_t begin, uint32_t end, State in, uint32_t limit,
                          bool last, Tally& t, uint32_t nblocks, int first_mcu, Out& out, Fail& fail) {
  const int nl = g.ncomp == 3 ? g.hs * g.vs : 1, bpm = blocks_per_mcu(g);
  const uint32_t ebits = 8u * (end - begin);
  Bits<Src> b{src, begin + (in.pos >> 3), end, 0, 0, 0};
  b.fill();
  b.skip((int)(in.pos & 7));
  uint32_t pos = in.pos;
  int k = (int)(in.sk & 63u), slot = (int)((in.sk >> 8) & 7u);
  uint32_t gb = WRITE ? t.blocks : 0u;
  if (WRITE) slot = (int)(gb % (uint32_t)bpm);  // (what the state holds at the fixed point; rows are addressed from gb alone)
  if (slot >= bpm) slot = 0;
  // (per-lane component indices select among scalars: no indexed private array, no scratch on the device)
  uint32_t dc0 = WRITE ? t.dc[0] : 0u, dc1 = WRITE ? t.dc[1] : 0u, dc2 = WRITE ? t.dc[2] : 0u;
  const int tdc0 = g.dc[0], tdc1 = g.dc[1], tdc2 = g.dc[2], tac0 = g.ac[0], tac1 = g.ac[1], tac2 = g.ac[2];
  int mcu = 0;
  if (WRITE && gb < nblocks) {
    mcu = first_mcu + (int)(gb / (uint32_t)bpm);
    int c;
    long long blk;
    block_of(g, mcu, slot, c, blk);
    out.begin(c, blk);
  }
  for (;;) {
    if (WRITE) {
      if (gb >= nblocks) break;
      if (last ? (k == 0 && pos > ebits) : pos >= limit) break;
    } else if (pos >= limit) {
      break;
    }
    b.fill();
    const int c = slot < nl ? 0 : slot - nl + 1;
    bool endblk = false;
    int ev = 0;
    if (k == 0) {
      const int s = symbol(b, tab[c == 0 ? tdc0 : (c == 1 ? tdc1 : tdc2)]);
      if (s < 0 || s > 11) {
        ev = BAD_CODE;
      } else {
        int diff = 0;
        if (s) {
          diff = extend(b.peek(s), s);
          b.skip(s);
        }
        dc0 += c == 0 ? (uint32_t)diff : 0u;
        dc1 += c == 1 ? (uint32_t)diff : 0u;
        dc2 += c == 2 ? (uint32_t)diff : 0u;
        if (WRITE && !out.put(0, (int)(c == 0 ? dc0 : (c == 1 ? dc1 : dc2)))) note(fail, gb, 1, BAD_RANGE);
        k = 1;
      }
    } else {
      const HuffDev& ac = tab[c == 0 ? tac0 : (c == 1 ? tac1 : tac2)];
      const int f = (int)(int16_t)(ac.lf[b.peek(LOOK)] >> 16);
      if (f) {  // code and value in one look-up
        k += (f >> 4) & 15;
        if (k > 63) {
          ev = BAD_INDEX;
        } else {
          b.skip(f & 15);
          if (WRITE && !out.put(k, f >> 8)) note(fail, gb, 1, BAD_RANGE);
          ++k;
        }
      } else {
        const int rs = symbol(b, ac);
        const int r = rs >> 4, s = rs & 15;
        if (rs < 0) {
          ev = BAD_CODE;
        } else if (s == 0) {
          if (r == 15) {
            k += 16;
            if (k > 63) ev = BAD_INDEX;
          } else if (r == 0) {
            endblk = true;
          } else {
            ev = BAD_EOB;
          }
        } else {
          k += r;
          if (k > 63) {
            ev = BAD_INDEX;
          } else if (s > 10) {
            ev = BAD_CODE;
          } else {
            const int v = extend(b.peek(s), s);
            b.skip(s);
            if (WRITE && !out.put(k, v)) note(fail, gb, 1, BAD_RANGE);
            ++k;
          }
        }
      }
      if (!ev && k > 63) endblk = true;
    }
    if (ev) {  // the recovery: skip one bit, end the block
      b.skip(1);
      endblk = true;
      if (WRITE) note(fail, gb, 0, ev);
    }
    pos = position(b, begin);
    if (endblk) {
      if (WRITE && pos > ebits) note(fail, gb, 2, OVERRUN);
      ++gb;
      k = 0;
      if (++slot == bpm) {
        slot = 0;
        ++mcu;
      }
      if (WRITE) {
        if (gb < nblocks) {
          int c2;
          long long blk;
          block_of(g, mcu, slot, c2, blk);
          out.begin(c2, blk);
        } else if (pos <= ebits) {  // behind the last block: eight or more real bits left?
          const uint32_t at = pos >> 3;
          const uint32_t next = at + ((pos & 7) ? (src.byte(begin + at) == 0xFF ? 2u : 1u) : 0u);
          if (next < end - begin) note(fail, gb - 1, 3, TRAILING);
        }
      }
    }
  }
  if (!WRITE) {
    t.blocks = gb;
    t.dc[0] = dc0;
    t.dc[1] = dc1;
    t.dc[2] = dc2;
  }
  State st;
  st.pos = pos >= ebits ? ebits : pos;
  st.sk = (uint32_t)k | ((uint32_t)slot << 8) | (pos >= ebits ? FED : 0u);
  return st;
}

JPEGX_HD inline uint32_t limit_of(const Cut& c, int j, uint32_t E) {
  const uint64_t hi = (uint64_t)(j + 1) * c.s;
  return 8u * (uint32_t)(hi < E ? hi : E);
}

// exclusive scan of the tallies, in place (the device runs its own over the LDS)
JPEGX_HD inline void scan_tallies(Sub* sub, int nsub) {
  Tally run = {0, {0, 0, 0}};
  for (int j = 0; j < nsub; ++j) {
    const Tally t = sub[j].t;
    sub[j].t = run;
    run.blocks += t.blocks;
    for (int c = 0; c < 3; ++c) run.dc[c] += t.dc[c];
  }
}

// A sink that writes nothing: what a speculative run is given.
struct NoOut {
  JPEGX_HD inline void begin(int, long long) {}
  JPEGX_HD inline bool put(int, int) { return true; }
};

// One split interval with the lanes as a loop.  sub: cut.nsub entries of workspace.  Out as in run(), plus `void zero()`, which
// clears the row begin() opened.  Returns the interval's Code with *rounds = the rounds taken (the empty one counted), or
// NOT_SYNCHRONISED with *rounds = max_rounds: nothing was written, the caller decodes serially.
template <class Src, class Out>
inline int decode_split(const Src& src, const Geometry& g, const HuffDev* tab, const Interval& I, const Cut& cut, int max_rounds, Sub* sub,
                        Out& out, int* rounds) {
  const uint32_t E = I.end - I.begin;
  const uint32_t nblocks = (uint32_t)I.nmcu * (uint32_t)blocks_per_mcu(g);
  NoOut none;
  Fail fail = {NO_KEY, CLEAN};
  for (int j = 0; j < cut.nsub; ++j) {
    sub[j].entry = j ? guess(src, I.begin, (uint32_t)j * cut.s) : State{0, 0};
    sub[j].exit = State{0xFFFFFFFFu, 0xFFFFFFFFu};
  }
  int r = 1;
  for (;; ++r) {
    if (r > max_rounds) {
      *rounds = max_rounds;
      return NOT_SYNCHRONISED;
    }
    // the entries of a round come from the previous round's exits: decide first, decode after
    bool any = r == 1;
    for (int j = cut.nsub - 1; j >= 1 && r > 1; --j) {
      const State want = sub[j - 1].exit;
      if (want.pos != sub[j].entry.pos || want.sk != sub[j].entry.sk) {
        sub[j].entry = want;
        sub[j].exit.pos = 0xFFFFFFFFu;  // (marks it for this round; a stored exit never has this position)
        any = true;
      }
    }
    if (!any) break;
    for (int j = 0; j < cut.nsub; ++j)
      if (sub[j].exit.pos == 0xFFFFFFFFu)
        sub[j].exit = run<false>(src, g, tab, I.begin, I.end, sub[j].entry, limit_of(cut, j, E), false, sub[j].t, 0, 0, none, fail);
  }
  *rounds = r;
  scan_tallies(sub, cut.nsub);
  for (uint32_t gb = 0; gb < nblocks; ++gb) {
    int c;
    long long blk;
    block_of(g, I.first_mcu + (int)(gb / (uint32_t)blocks_per_mcu(g)), (int)(gb % (uint32_t)blocks_per_mcu(g)), c, blk);
    out.begin(c, blk);
    out.zero();
  }
  for (int j = 0; j < cut.nsub; ++j)
    run<true>(src, g, tab, I.begin, I.end, sub[j].entry, limit_of(cut, j, E), j == cut.nsub - 1, sub[j].t, nblocks, I.first_mcu, out, fail);
  return fail.key == NO_KEY ? CLEAN : fail.code;
}

// ---- the host form: plain memory, the lanes as a loop ----------------------------------------------------------------------------

struct MemSrc {  // the file bytes of a record
  const uint8_t* base;
  unsigned byte(uint32_t pos) const { return base[pos]; }
};

// the coefficient area of one image in plain memory, as both decoders address it
struct MemPlanes {
  const uint16_t* qt;  // [3][64], natural order
  int16_t* plane[3];
  void set(const uint16_t* q, int16_t* coef, const Desc& d) {
    qt = q;
    plane[0] = coef;
    plane[1] = plane[2] = nullptr;
    for (int c = 1; c < d.ncomp; ++c) plane[c] = plane[c - 1] + (size_t)d.bw[c - 1] * d.bh[c - 1] * 64;
  }
};
inline bool in_range(int v, unsigned q) {
  const int t = (int)((unsigned)v * q);
  return t <= MAX_ABS_DEQUANT && t >= -MAX_ABS_DEQUANT;
}

// the serial decoder's sink with the device sink's rules: a block is stored whole at its end and its range judged there
struct RowSink {
  MemPlanes m;
  const uint16_t* q;
  int16_t* out;
  int val[64];
  void begin(int c, long long blk) {
    q = m.qt + 64 * c;
    out = m.plane[c] + blk * 64;
    memset(val, 0, sizeof(val));
  }
  bool put(int k, int v) {
    val[jpegx::detail::NATURAL[k]] = v;
    return true;
  }
  bool end() {
    bool ok = true;
    for (int i = 0; i < 64; ++i) {
      out[i] = (int16_t)val[i];
      ok = ok && in_range(val[i], q[i]);
    }
    return ok;
  }
};

// the write pass's sink
struct RowOut {
  MemPlanes m;
  const uint16_t* q;
  int16_t* out;
  void begin(int c, long long blk) {
    q = m.qt + 64 * c;
    out = m.plane[c] + blk * 64;
  }
  void zero() { memset(out, 0, 128); }
  bool put(int k, int v) {
    const int nat = jpegx::detail::NATURAL[k];
    out[nat] = (int16_t)v;
    return in_range(v, q[nat]);
  }
};

inline Geometry geometry_of(const Desc& d, const ScanHeader& h) {
  Geometry g;
  g.ncomp = d.ncomp;
  g.hs = d.hs;
  g.vs = d.vs;
  g.mx = d.bw[0] / d.hs;
  for (int c = 0; c < 3; ++c) {
    g.bw[c] = d.bw[c];
    g.dc[c] = h.dc_tab[c];
    g.ac[c] = h.ac_tab[c];
  }
  return g;
}

// One interval of a checked record by the rule of the cut: split, or serial when it is short or does not synchronise in
// max_rounds.  *rounds: 0 (not split), r, or -max_rounds (serial after the cap).
inline int decode_interval_host(const uint8_t* file, const Geometry& g, const HuffDev* tab, const Interval& I, const MemPlanes& m,
                                uint32_t split_bytes, int max_rounds, int* rounds) {
  const Cut cut = cut_of(I.end - I.begin, split_bytes);
  *rounds = 0;
  if (cut.nsub) {
    std::unique_ptr<Sub[]> sub(new Sub[(size_t)cut.nsub]);
    RowOut out;
    out.m = m;
    out.q = m.qt;
    out.out = m.plane[0];
    const int code = decode_split(MemSrc{file}, g, tab, I, cut, max_rounds, sub.get(), out, rounds);
    if (code != NOT_SYNCHRONISED) return code;
    *rounds = -max_rounds;
  }
  RowSink sink;
  sink.m = m;
  return decode_interval(MemSrc{file}, g, tab, I.begin, I.end, I.first_mcu, I.nmcu, sink);
}

// A whole scan record -> [tables | coefficients] (record_bytes(d) <= out_bytes), the image's status and its rounds word: what
// the device entry writes for one image.  d: the host descriptor, as checked by the caller (geometry consistent with itself).
inline void decode_record_host(const uint8_t* rec, size_t avail, const Desc& d, uint32_t split_bytes, int max_rounds, uint8_t* out,
                               int32_t* status, int32_t* rounds) {
  *status = BAD_RECORD;
  *rounds = 0;
  ScanHeader h;
  if (avail < sizeof(h)) return;
  memcpy(&h, rec, sizeof(h));
  const long long nint = intervals_of(d);
  if (!header_fits(h, nint, avail)) return;
  const Geometry g = geometry_of(d, h);
  const HuffDev* tab = reinterpret_cast<const HuffDev*>(rec + TAB_OFF);
  const Interval* ivl = reinterpret_cast<const Interval*>(rec + ivl_off(h.ntables));
  const uint8_t* file = rec + file_off(h.ntables, h.nintervals);
  memcpy(out, rec + QT_OFF, TABLE_BYTES);
  MemPlanes m;
  m.set(reinterpret_cast<const uint16_t*>(rec + QT_OFF), reinterpret_cast<int16_t*>(out + TABLE_BYTES), d);
  const long long mcus = mcus_of(d), per = d.restart > 0 ? (d.restart < mcus ? d.restart : mcus) : mcus;
  int worst = CLEAN, most = 0, gave_up = 0;
  for (long long i = 0; i < nint; ++i) {
    const Interval I = ivl[i];
    const long long first = i * per;
    int code = BAD_RECORD, r = 0;
    if (I.first_mcu == first && I.nmcu == (per < mcus - first ? per : mcus - first) && I.begin <= I.end && I.end <= h.file_bytes)
      code = decode_interval_host(file, g, tab, I, m, split_bytes, max_rounds, &r);
    worst = code > worst ? code : worst;
    if (r < 0) gave_up = -r;
    most = r > most ? r : most;
  }
  *status = worst;
  *rounds = gave_up ? -gave_up : most;
}

}  // namespace split
}  // namespace scan
}  // namespace jpegx
