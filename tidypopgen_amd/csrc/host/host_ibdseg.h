// host_ibdseg.h -- the per-pair state machine of include/tpg.h "IBD segments", written once for the host and the device: it
// consumes the loci of a pair 32 at a time as three words (bad, typed, brk) and hands every closed segment to a sink.  The
// lanes of tpg_ibd_scan_kernel (ibdseg.hip) call these very functions; the stand-alone program of tests/host/ibdseg_san.cpp
// runs them under the host sanitizers.  Also the breaks between neighbouring loci and the genome length, which only the host
// computes.  Everything is an integer.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define TPG_IBD_FN __host__ __device__ static inline
#else
#define TPG_IBD_FN static inline
#endif

// O(1) state of a pair.  A CHAIN is one or more closed stretches already joined; it exists only while it waits for the stretch
// behind the one bad locus that follows it (whether that joint holds is known when that stretch closes), so its last locus
// need not be kept: it is two loci before the open stretch, or before the locus that ends the wait.
struct HostIbdState {
  int32_t s = -1;      // first locus of the open clean stretch, -1: none
  int32_t c = 0;       // typed loci of the open stretch
  int32_t first = -1;  // first locus of the waiting chain, -1: none
  int32_t typed = 0;   // typed loci of the chain, its bridged bad loci included
  int32_t err = 0;     // bridged bad loci of the chain
};

// step 4: is the segment reported?  max_err < 0: no limit
TPG_IBD_FN bool host_ibd_reported(int32_t n_typed, int64_t length, int32_t n_err, int64_t min_snp, int64_t min_length, int64_t max_err) {
  return n_typed >= min_snp && length >= min_length && (max_err < 0 || n_err <= max_err);
}

// `ntyped` typed loci of a clean piece that begins at locus j and crosses no break
TPG_IBD_FN void host_ibd_clean(HostIbdState& st, int32_t j, int32_t ntyped) {
  if (st.s < 0) {  // (a chain that waits began two loci before j: the only way to get here with one)
    st.s = j;
    st.c = 0;
  }
  st.c += ntyped;
}

// the open stretch [st.s, e] closes: by the bad locus e + 1 (brk[e] is false then), or by brk[e].  B = bridge_min_snp.
// sink(first, last, n_typed, n_err) takes a segment.
template <class Sink>
TPG_IBD_FN void host_ibd_close(HostIbdState& st, int32_t e, bool by_bad, int32_t B, Sink& sink) {
  if (st.first >= 0 && st.c >= B) {  // the joint with the chain holds (the chain's side was checked when it began to wait)
    st.typed += 1 + st.c;
    st.err += 1;
  } else {
    if (st.first >= 0) sink(st.first, st.s - 2, st.typed, st.err);
    st.first = st.s;
    st.typed = st.c;
    st.err = 0;
  }
  if (!(by_bad && B > 0 && st.c >= B)) {  // nothing can join behind this stretch
    sink(st.first, e, st.typed, st.err);
    st.first = -1;
  }
  st.s = -1;
}

// locus j is bad, or brk[j] is set (the last locus of the panel counts as a break)
template <class Sink>
TPG_IBD_FN void host_ibd_event(HostIbdState& st, int32_t j, bool bad, bool typed, bool brk, int32_t B, Sink& sink) {
  if (bad) {
    if (st.s >= 0) {
      host_ibd_close(st, j - 1, true, B, sink);
    } else if (st.first >= 0) {  // the second bad locus in a row: no stretch begins two loci behind the chain
      sink(st.first, j - 2, st.typed, st.err);
      st.first = -1;
    }
    if (brk && st.first >= 0) {  // a break next to the bad locus
      sink(st.first, j - 1, st.typed, st.err);
      st.first = -1;
    }
  } else {
    host_ibd_clean(st, j, typed ? 1 : 0);
    if (brk) host_ibd_close(st, j, false, B, sink);
  }
}

// A clean stretch that begins and ends inside one word has at most 32 typed loci.  With min_snp >= 33, and bridge_min_snp
// >= 33 where bridging is on, it can neither be reported nor be joined to anything: all it does is end the wait of a chain.
// host_ibd_word may then skip such stretches without looking at them (skip_short).
TPG_IBD_FN bool host_ibd_skip_short(int64_t min_snp, int64_t bridge_min_snp) {
  return min_snp >= 33 && (bridge_min_snp == 0 || bridge_min_snp >= 33);
}

// the loci j0 .. j0 + 31: bit b of a word belongs to locus j0 + b.  Loci behind the last of the panel are neither bad nor
// typed and have no break: they open a stretch that never closes.  A word without bad locus and break costs one popcount.
// skip_short = host_ibd_skip_short(...): once nothing is open and nothing waits, everything up to the last bad locus or
// break of the word is short stretches, and the walk goes on behind it.
template <class Sink>
TPG_IBD_FN void host_ibd_word(HostIbdState& st, int32_t j0, uint32_t bad, uint32_t typed, uint32_t brk, int32_t B, bool skip_short,
                              Sink& sink) {
  uint32_t ev = bad | brk;
  if (ev == 0) {
    host_ibd_clean(st, j0, __builtin_popcount(typed));
    return;
  }
  int p = 0;  // the loci below p are done
  while (ev) {
    if (skip_short && st.s < 0 && st.first < 0) {
      p = 32 - __builtin_clz(ev);
      break;
    }
    const int b = __builtin_ctz(ev);
    ev &= ev - 1;
    if (b > p) host_ibd_clean(st, j0 + p, __builtin_popcount(typed & ((1u << b) - 1u) & ~((1u << p) - 1u)));
    const bool isbad = (bad >> b) & 1u;
    host_ibd_event(st, j0 + b, isbad, (typed >> b) & 1u, (brk >> b) & 1u, B, sink);
    p = b + 1;
    if (isbad && st.first < 0) {  // nothing open, nothing waits: the bad loci that follow at once change nothing
      const uint32_t clean_above = ~bad & ~((2u << b) - 1u);
      if (clean_above == 0) return;  // bad up to the end of the word
      p = __builtin_ctz(clean_above);
      ev &= ~((1u << p) - 1u);
    }
  }
  if (p < 32) host_ibd_clean(st, j0 + p, __builtin_popcount(typed >> p));
}

// bad and typed of one locus from the two codes (0, 1, 2, 3 = missing); kind 1: opposite homozygotes, kind 2: codes differ
TPG_IBD_FN void host_ibd_locus_bits(int kind, int ca, int cb, bool& bad, bool& typed) {
  typed = ca != 3 && cb != 3;
  bad = typed && (kind == 1 ? (ca + cb == 2 && ca != cb) : ca != cb);
}

// Step 1 on the host.  brk_words (may be NULL): ceil(m / 32) zeroed words, bit j & 31 of word j >> 5 = brk[j], and bit m - 1
// set; *length (may be NULL): the sum over the break-free regions of pos[last] - pos[first].  Returns -1, or the first locus
// whose position is below its predecessor's on the same chromosome.
static inline int64_t host_ibd_breaks(const int32_t* chrom, const int64_t* pos, int64_t m, int64_t max_gap, uint32_t* brk_words,
                                      int64_t* length) {
  uint64_t total = 0;
  int64_t region = 0;  // first locus of the break-free region
  for (int64_t j = 0; j < m; j++) {
    bool brk = j == m - 1;
    if (!brk) {
      const bool same = chrom[j] == chrom[j + 1];
      if (same && pos[j + 1] < pos[j]) return j + 1;
      brk = !same || (uint64_t)pos[j + 1] - (uint64_t)pos[j] > (uint64_t)max_gap;
    }
    if (brk) {
      if (brk_words) brk_words[j >> 5] |= 1u << (j & 31);
      total += (uint64_t)pos[j] - (uint64_t)pos[region];
      region = j + 1;
    }
  }
  if (length) *length = (int64_t)total;
  return -1;
}
