// Part of encode.hip (included there, inside its anonymous namespace): K4: CTable helpers and the sequence chain kernels (segment functions over state sets).

// ------------------------------------------------------------------ K4: state chains
struct LdsCTable {
  const uint16_t *state_table;
  const uint32_t *tt;  // {deltaFindState, deltaNbBits} pairs
  unsigned log;
};

// copies one context's CTable (zstd word layout) into LDS; all 64 lanes of the wave
template <class M>
__device__ __forceinline__ LdsCTable stage_ctable(uint32_t *lds, const uint32_t *__restrict__ tbl) {
  const unsigned log = tbl[0] & 0xFFFFu;
  const unsigned words = 1u + (1u << (log - 1)) + 2u * M::A;
  for (unsigned i = fq_lane(); i < words; i += 64) lds[i] = tbl[i];
  __syncthreads();
  LdsCTable t;
  t.log = log;
  t.state_table = reinterpret_cast<const uint16_t *>(lds) + 2;
  t.tt = lds + 1 + (1u << (log - 1));
  return t;
}

// FSE_encodeSymbol (zstd fse.h) on the LDS copy: returns the packed (nb << 12 | bits)
__device__ __forceinline__ unsigned chain_step(const LdsCTable &t, unsigned &x, unsigned sym) {
  const int dfs = (int)t.tt[2 * sym];
  const unsigned dnb = t.tt[2 * sym + 1];
  const unsigned nb = (x + dnb) >> 16;
  const unsigned out = (nb << 12) | (x & ((1u << nb) - 1u));
  x = t.state_table[(int)(x >> nb) + dfs];
  return out;
}

// the one cell of a symbol with normalised count 1 or -1: stateTable[1 + deltaFindState]
__device__ __forceinline__ unsigned reset_state(const LdsCTable &t, unsigned sym) {
  return t.state_table[1 + (int)t.tt[2 * sym]];
}

// ---- sequence chains -------------------------------------------------------------------
// Sequence contexts have no single-state symbols, so a chain cannot be cut "for free", and a
// tANS encoder state never forgets its history.  But it forgets MOST of it: pushed through the
// same symbols, the 2^log possible states collapse onto a small set (about 150 survivors
// after 128 symbols for exactly uniform counts, a few dozen otherwise), because every
// transition x -> stateTable[(x >> nb) + delta] merges the states that share x >> nb.  The
// chain of a context is therefore cut into segments of S symbols and coded in three exact steps:
//  (A) k_seq_setfunc: a wave computes F: entry state -> exit state for EVERY possible entry
//      state.  It starts with all 2^log states spread over the lanes, and at a few points (after
//      4, 16, 48, 128, 512, 2048, ... symbols) replaces the states it carries by the distinct
//      ones ("classes"), remembering which class every entry state fell into.  After the first
//      hundred symbols a step costs 1-3 LDS gathers per wave for 64 lanes, from ~2048 symbols on
//      one -- so the wave walks on through a GROUP of up to 8 consecutive segments and writes
//      the function "entry state of the group -> state here" at every segment boundary.
//  (B) k_seq_resolve: entry state of every segment; a group's functions all start at the group's
//      entry state (one round of independent loads), x <- F_last[x] from group to group.
//  (C) k_seq_emit: every lane walks ONE segment from its now-known entry state and writes the
//      packed (nb, bits) of every symbol, 64 symbols and one cache line of output per round; 64 segments of a context per wave.
// All three read the context's one-symbol transition table next[s][x] from LDS (tables.hip
// builds it once per handle).  Exact by construction: no speculation, nothing to verify.
// (SETS_WAVES, SETS_WAVES2, SETS_ROUNDS, SETS_MAX_GROUP, SETS_BLOCK, SEQ_CAND_MAX: enc_plan.h, the host sizes scratch by them)
constexpr unsigned SETS_MAX_CLASSES = 512;  // above this a segment keeps carrying every state

// Hand-over of collapsed groups (two-symbol path).  After a prefix of P segments the states a group still carries are
// few (19-40 after 2048 symbols, fewer than 10 from 8192 on), and a 64-lane gather per step walks mostly spare lanes.  A
// wave of k_seq_setfunc that stands at n <= cap classes behind the prefix writes them out as the group's CANDIDATES and
// takes its next group; k_seq_candwalk walks the rest of the group with one lane per candidate, in rows of 16 lanes that
// get their symbols' table rows by DPP broadcast (W / 16 rows per group, 64 / W groups per wave), and needs nothing but
// the context's table in LDS; k_seq_resolve finds a group entry's candidate through F_P.  (The candidates keep merging --
// a median of 16 / 10 / 7 distinct states behind 4096 / 8192 / 12288 symbols at log 11 -- and rows dealt anew at every
// segment boundary, one per 16 distinct states, were built and measured: 45 % fewer gathers, the same step.  DESIGN.md 8.)
constexpr unsigned SEQ_CAND_KEPT = 0xFFFFu;  // cand0[group][0] of a group that kept its functions (no state: states are even)
constexpr unsigned CANDW_WAVES = 8;          // waves of a k_seq_candwalk workgroup
struct SeqHandover {
  unsigned W;        // candidate slots per group: 16, 32 or 64 (0: nothing is handed over)
  unsigned cap, P;   // a group is handed over with at most cap classes behind its first P segments
  uint16_t *cand0;   // [first function of the group][W] the candidates behind the prefix, padded with the last one
  uint16_t *cand;    // [function][W] candidate k's state behind that segment (segments P.. of a handed-over group)
  unsigned *counts;  // groups handed over, groups kept (of the block)
};

template <unsigned MAXC_, unsigned BMW_>
struct SetsWaveLdsT {
  static constexpr unsigned MAXC = MAXC_, BMW = BMW_;
  uint32_t bm[BMW];       // bitmap over the states (size <= 32 * BMW)
  uint16_t wpre[BMW];     // set bits before every bitmap word
  uint16_t list[MAXC];    // class -> state, as (state - size) * 2
  uint16_t tmp[MAXC];     // old class -> new class during a merge
  uint16_t m[MAXC];       // first-level class -> current class
};
using SetsWaveLds = SetsWaveLdsT<SETS_MAX_CLASSES, 128>;    // any log <= 12
// log <= 11 (the two-symbol kernel): 3456 B per wave, 16 waves + the 64 KB table = 118 KB, which
// leaves 42 KB of a CU's LDS to the kernels of the other lanes -- the quality K1 and K3 need 36 KB
// each and could not run beside a workgroup of this kernel while it took 125 KB
using SetsWaveLds11 = SetsWaveLdsT<SETS_MAX_CLASSES, 64>;

// Segments a k_seq_setfunc wave walks in one go ("group") for a chain with nf functions: as many
// as keep >= gmin groups in the chain (a workgroup's waves all busy), at most qmax.
__device__ __forceinline__ unsigned seq_group_of(unsigned nf, unsigned qmax, unsigned gmin) {
  return min(max((nf + gmin - 1) / gmin, 1u), qmax);
}

// plan[]: its layout, SEGPLAN_WORDS and SEQ_ITEM_GROUPS stand in enc_plan.h
// items of a chain with nl groups (0: the chain is short, k_seq_resolve walks its groups itself)
__device__ __forceinline__ unsigned seq_items_of(unsigned nl) { return nl > SEQ_ITEM_GROUPS ? (nl + SEQ_ITEM_GROUPS - 1) / SEQ_ITEM_GROUPS : 0u; }

__global__ void __launch_bounds__(256)
k_seq_segplan(const uint32_t *__restrict__ arrays, unsigned S, unsigned qmax, unsigned gmin, unsigned wpg,
              uint32_t *__restrict__ plan) {
  constexpr unsigned B = SeqModel::B;
  __shared__ unsigned s_nseg[B];
  const unsigned c = threadIdx.x;
  const unsigned n = arrays[c];
  s_nseg[c] = (n + S - 1) / S;
  __syncthreads();
  unsigned fi = 0, fs = 0, sg = 0, ei = 0, ci = 0;
  for (unsigned o = 0; o < c; o++) {
    const unsigned ns = s_nseg[o], nf = ns ? ns - 1 : 0, Q = seq_group_of(nf, qmax, gmin), nl = (nf + Q - 1) / Q;
    fi += (nl + wpg - 1) / wpg; fs += nf; sg += ns; ei += (ns + 63) / 64; ci += seq_items_of(nl);
  }
  uint32_t *fitem = plan, *fseg = plan + (B + 1), *seg = plan + 2 * (B + 1), *eitem = plan + 3 * (B + 1), *citem = plan + 4 * (B + 1);
  fitem[c] = fi; fseg[c] = fs; seg[c] = sg; eitem[c] = ei; citem[c] = ci;
  if (c == 0) plan[5 * (B + 1)] = 0;  // step A's work counter
  if (c == B - 1) {
    const unsigned ns = s_nseg[c], nf = ns ? ns - 1 : 0, Q = seq_group_of(nf, qmax, gmin), nl = (nf + Q - 1) / Q;
    fitem[B] = fi + (nl + wpg - 1) / wpg; fseg[B] = fs + nf; seg[B] = sg + ns; eitem[B] = ei + (ns + 63) / 64; citem[B] = ci + seq_items_of(nl);
  }
}

// last context c with base[c] <= item (base is an exclusive prefix with B + 1 entries)
__device__ __forceinline__ unsigned seq_item_ctx(const uint32_t *__restrict__ base, unsigned item) {
  unsigned lo = 0, hi = SeqModel::B - 1;
  while (lo < hi) {
    const unsigned mid = lo + ((hi - lo + 1) >> 1);
    if (base[mid] <= item) lo = mid; else hi = mid - 1;
  }
  return lo;
}

__device__ __forceinline__ unsigned sets_incl_scan(unsigned v) {
  const unsigned lane = fq_lane();
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const unsigned o = __shfl_up(v, d);
    if (lane >= (unsigned)d) v += o;
  }
  return v;
}

// The segment's symbols travel 1024 at a time: lane l holds symbols 16 l .. 16 l + 15 of the
// block, a word of four symbols is fetched with v_readlane (w: uniform word index in the segment).
__device__ __forceinline__ unsigned sets_word(const uint4 cur, unsigned w) {
  const unsigned g = (w >> 2) & 63u, q = w & 3u;
  const unsigned a = __builtin_amdgcn_readlane(cur.x, g), b = __builtin_amdgcn_readlane(cur.y, g),
                 c = __builtin_amdgcn_readlane(cur.z, g), d = __builtin_amdgcn_readlane(cur.w, g);
  return q == 0 ? a : q == 1 ? b : q == 2 ? c : d;
}

// number of distinct states marked in L.bm; fills L.wpre
template <class LT>
__device__ __forceinline__ unsigned sets_count(LT &L, unsigned nw) {
  const unsigned lane = fq_lane();
  const unsigned c0 = lane < nw ? __popc(L.bm[lane]) : 0u;
  const unsigned p0 = sets_incl_scan(c0), t0 = __builtin_amdgcn_readlane(p0, 63);
  L.wpre[lane] = (uint16_t)(p0 - c0);
  unsigned t1 = 0;
  if (LT::BMW > 64) {
    const unsigned c1 = lane + 64 < nw ? __popc(L.bm[lane + 64]) : 0u;
    const unsigned p1 = sets_incl_scan(c1);
    t1 = __builtin_amdgcn_readlane(p1, 63);
    L.wpre[lane + 64] = (uint16_t)(t0 + p1 - c1);
  }
  fq_lds_wave_sync();
  return t0 + t1;
}
template <class LT>
__device__ __forceinline__ unsigned sets_rank(const LT &L, unsigned xi) {
  return (unsigned)L.wpre[xi >> 5] + __popc(L.bm[xi >> 5] & ((1u << (xi & 31u)) - 1u));
}
template <class LT>
__device__ __forceinline__ void sets_clear(LT &L) {
  L.bm[fq_lane()] = 0;
  if (LT::BMW > 64) L.bm[fq_lane() + 64] = 0;
  fq_lds_wave_sync();
}

// byte offsets of the table rows the four symbols of a word select: one row per symbol, or
// (TWO) one row of the two-symbol table per symbol pair
template <bool TWO>
__device__ __forceinline__ void sets_rows(unsigned word, unsigned log, unsigned (&row)[TWO ? 2 : 4]) {
  if (TWO) {
    row[0] = ((word & 3u) | ((word >> 6) & 0xCu)) << (log + 1);
    row[1] = (((word >> 16) & 3u) | ((word >> 22) & 0xCu)) << (log + 1);
  } else {
#pragma unroll
    for (int i = 0; i < 4; i++) row[i] = ((word >> (8 * i)) & 3u) << (log + 1);
  }
}

// two-symbol table: the lane's 16 symbols as eight 16-bit row offsets, two per dword
__device__ __forceinline__ uint4 sets_pack_rows(const uint4 cur, unsigned log) {
  auto pk = [&](unsigned w) {
    return (((w & 3u) | ((w >> 6) & 0xCu)) << (log + 1)) | (((((w >> 16) & 3u) | ((w >> 22) & 0xCu)) << (log + 1)) << 16);
  };
  return make_uint4(pk(cur.x), pk(cur.y), pk(cur.z), pk(cur.w));
}

// One gather of the two-symbol walk, table at LDS address 0 (k_seq_setfunc has no static LDS: tests/test_build_invariants.py):
// the row offset is one 16-bit half of a scalar register (two rows per register, sets_pack_rows) and is picked by the ADD
// itself (SDWA word select on the scalar operand), the LDS address is the sum -- add, read, wait: three instructions per
// gather where the compiler's version had five (s_and / s_lshr for the half, s_add for the table's base).
typedef __attribute__((address_space(3))) const uint16_t fq_lds_u16;
template <int HALF>
__device__ __forceinline__ unsigned sets_gather2(unsigned rowpair, unsigned y) {
  unsigned addr;
  if (HALF == 0)
    asm("v_add_u32_sdwa %0, %1, %2 dst_sel:DWORD dst_unused:UNUSED_PAD src0_sel:WORD_0 src1_sel:DWORD" : "=v"(addr) : "s"(rowpair), "v"(y));
  else
    asm("v_add_u32_sdwa %0, %1, %2 dst_sel:DWORD dst_unused:UNUSED_PAD src0_sel:WORD_1 src1_sel:DWORD" : "=v"(addr) : "s"(rowpair), "v"(y));
  return *reinterpret_cast<fq_lds_u16 *>((uintptr_t)addr);
}

// n classes (states in L.list) walked through words [w0, w1) of the segment, M per lane
template <int M, bool TWO, class LT>
__device__ __forceinline__ void sets_walk(LT &L, unsigned n, const char *tbase, unsigned log,
                                          const uint4 cur, const uint4 rows, unsigned w0, unsigned w1) {
  const unsigned lane = fq_lane();
  unsigned y[M];
#pragma unroll
  for (int j = 0; j < M; j++) {
    const unsigned i = lane + 64u * j;
    y[j] = L.list[i < n ? i : n - 1];  // spare slots shadow the last class
  }
  auto step_word = [&](unsigned word) {
    unsigned row[TWO ? 2 : 4];
    sets_rows<TWO>(word, log, row);
#pragma unroll
    for (int i = 0; i < (TWO ? 2 : 4); i++) {
#pragma unroll
      for (int j = 0; j < M; j++) y[j] = *reinterpret_cast<const uint16_t *>(tbase + (row[i] + y[j]));
    }
  };
  w0 = fq_uniform(w0); w1 = fq_uniform(w1);  // (wave-uniform by construction; said so, the loops below run on scalar counters)
  if ((w0 | w1) & 3u) {  // only the first two ranges of a segment: [0, 1) and [1, 4)
    for (unsigned w = w0; w < w1; w++) step_word(sets_word(cur, w));
  } else if (TWO) {  // whole groups of 16 symbols = eight prepared row offsets of lane g
    for (unsigned g = w0 >> 2; g < (w1 >> 2); g++) {
      const unsigned gi = g & 63u;
      const unsigned r[4] = {(unsigned)__builtin_amdgcn_readlane(rows.x, gi), (unsigned)__builtin_amdgcn_readlane(rows.y, gi),
                             (unsigned)__builtin_amdgcn_readlane(rows.z, gi), (unsigned)__builtin_amdgcn_readlane(rows.w, gi)};
#pragma unroll
      for (int i = 0; i < 4; i++) {
#pragma unroll
        for (int j = 0; j < M; j++) y[j] = sets_gather2<0>(r[i], y[j]);
#pragma unroll
        for (int j = 0; j < M; j++) y[j] = sets_gather2<1>(r[i], y[j]);
      }
    }
  } else {
    for (unsigned g = w0 >> 2; g < (w1 >> 2); g++) {
      const unsigned gi = g & 63u;
      const unsigned a = __builtin_amdgcn_readlane(cur.x, gi), b = __builtin_amdgcn_readlane(cur.y, gi),
                     c = __builtin_amdgcn_readlane(cur.z, gi), d = __builtin_amdgcn_readlane(cur.w, gi);
      step_word(a); step_word(b); step_word(c); step_word(d);
    }
  }
#pragma unroll
  for (int j = 0; j < M; j++) {
    const unsigned i = lane + 64u * j;
    if (i < n) L.list[i] = (uint16_t)y[j];
  }
  fq_lds_wave_sync();
}

// bitmap index of a carried state: XO = (state - size) * 2 (sequence kernels), else the state itself
template <bool XO>
__device__ __forceinline__ unsigned sets_idx(unsigned v, unsigned size) { return XO ? v >> 1 : v - size; }

// merge of equal states among the n classes of L.list; returns the new class count.  Skipped
// (list untouched) when it would not lower the number of gathers per step (force: the number of classes).
template <bool XO, class LT>
__device__ __forceinline__ unsigned sets_merge(LT &L, unsigned n, unsigned n1, unsigned nw, unsigned size, bool force = false) {
  const unsigned lane = fq_lane();
  sets_clear(L);
  for (unsigned i = lane; i < n; i += 64) {
    const unsigned xi = sets_idx<XO>(L.list[i], size);
    atomicOr(&L.bm[xi >> 5], 1u << (xi & 31u));
  }
  fq_lds_wave_sync();
  const unsigned nn = sets_count(L, nw);
  if (force ? nn >= n : (nn + 63) / 64 >= (n + 63) / 64) return n;
  unsigned st[LT::MAXC / 64];
#pragma unroll
  for (unsigned j = 0; j < LT::MAXC / 64; j++) {
    const unsigned i = lane + 64u * j;
    st[j] = i < n ? (unsigned)L.list[i] : 0u;
    if (i < n) L.tmp[i] = (uint16_t)sets_rank(L, sets_idx<XO>(st[j], size));
  }
  fq_lds_wave_sync();
#pragma unroll
  for (unsigned j = 0; j < LT::MAXC / 64; j++) {
    const unsigned i = lane + 64u * j;
    if (i < n) L.list[L.tmp[i]] = (uint16_t)st[j];  // equal states write the same value
  }
  for (unsigned i = lane; i < n1; i += 64) L.m[i] = L.tmp[L.m[i]];
  fq_lds_wave_sync();
  return nn;
}

// Step A.  PER0 = states per lane at the start: 32 covers log <= 11, 64 covers log 12.
// TWO: two symbols per gather through the context's 64 KB two-symbol table (log <= 11).
// Registers: the two-symbol kernel is held to 96 VGPRs (five waves per SIMD; it spills 8 more
// registers of its rarely run merge code than at 128).  A workgroup is 4 waves per SIMD: at 128
// VGPRs they filled the SIMD's register file and NOTHING else could run on a CU while this
// kernel held it -- its time simply added to the step.  With 96, waves of the other lanes'
// kernels fit beside it: 66.9 -> 70.8 GB/s (80 VGPRs: 68.8; 64: 65.7).
template <unsigned PER0, bool TWO>
__global__ void __launch_bounds__((TWO ? SETS_WAVES2 : SETS_WAVES) * 64, TWO ? 5 : 1)
k_seq_setfunc(const uint8_t *__restrict__ sorted_sym, const uint32_t *__restrict__ arrays,
              const uint32_t *__restrict__ plan, const uint32_t *__restrict__ logs,
              const uint16_t *__restrict__ next, unsigned next_stride, const uint16_t *__restrict__ pow, unsigned pow_stride,
              unsigned S, unsigned qmax, unsigned gmin,
              unsigned rounds, unsigned fstride, uint16_t *__restrict__ fbuf, unsigned *__restrict__ work_counter, unsigned table_bytes,
              const SeqHandover H) {
  constexpr unsigned WAVES = TWO ? SETS_WAVES2 : SETS_WAVES;
  // ALL of the kernel's LDS is the dynamic block, the context's table first: next[4][size] (TWO: next2[16][size]) sits at LDS
  // address 0, so a gather's address is row + state with nothing added (with the per-wave buffers as static LDS in front of
  // it the compiler spent one s_add per gather on the table's base); behind it the waves' set buffers and two words
  using LT = typename std::conditional<TWO, SetsWaveLds11, SetsWaveLds>::type;
  extern __shared__ uint32_t lds[];
  LT *wl = reinterpret_cast<LT *>(reinterpret_cast<char *>(lds) + table_bytes);
  unsigned &s_next = *reinterpret_cast<unsigned *>(wl + WAVES), &s_item = *(reinterpret_cast<unsigned *>(wl + WAVES) + 1);
  constexpr unsigned B = SeqModel::B;
  const uint32_t *fitem = plan, *fseg = plan + (B + 1);
  const unsigned wave = threadIdx.x >> 6, lane = fq_lane();
  LT &L = wl[wave];
  const char *tbase = reinterpret_cast<const char *>(lds);
  const unsigned sub_blocks = S / SETS_BLOCK;  // 1024-symbol loads per segment
  const unsigned n_items = fitem[B];
  unsigned loaded = 0xFFFFFFFFu;  // context whose table is in LDS
  // Persistent workgroups (one per CU, 118 KB of LDS with the two-symbol table): items are
  // (context, group of WAVES * SETS_ROUNDS segments), taken from a global counter, so a
  // workgroup that has found a CU keeps it until the work is gone.
  for (;;) {
    __syncthreads();  // every wave is done with the previous item's table and queue
    if (threadIdx.x == 0) { s_item = atomicAdd(work_counter, 1u); s_next = WAVES; }
    __syncthreads();
    const unsigned item = s_item;
    if (item >= n_items) break;
    const unsigned c = seq_item_ctx(fitem, item);
    const unsigned log = logs[c], size = 1u << log;
    if (c != loaded) {  // (4 or 16) * size u16 entries, a multiple of 16 bytes
      const uint4 *src = reinterpret_cast<const uint4 *>(next + (size_t)c * next_stride);
      uint4 *dst = reinterpret_cast<uint4 *>(lds);
      for (unsigned e = threadIdx.x; e < (TWO ? 2 * size : size / 2); e += WAVES * 64) dst[e] = src[e];
      loaded = c;
      __syncthreads();
    }
    const unsigned nf = fseg[c + 1] - fseg[c], Q = seq_group_of(nf, qmax, gmin), nl = (nf + Q - 1) / Q;
    // A wave walks a GROUP of up to Q consecutive segments in one go and writes the function
    // "entry state of the group -> state behind segment j" at every segment boundary: the state
    // sets keep shrinking along the group (one gather per step from ~2048 symbols on), while a
    // fresh start pays ~1500 gathers for its first 2048 symbols.  The item's groups [k0, k_end)
    // of the chain go to whichever wave is free.
    const unsigned k0 = (item - fitem[c]) * (WAVES * rounds), k_end = min(k0 + WAVES * rounds, nl);
    const unsigned per = max(size >> 6, 1u), nw = max(size >> 5, 1u);
    for (unsigned k = k0 + wave; k < k_end;) {
      const unsigned s0 = k * Q, nblk = min(Q, nf - s0) * sub_blocks, w_end = nblk * (SETS_BLOCK / 4);
      const uint4 *gseg = reinterpret_cast<const uint4 *>(sorted_sym + arrays[B + c] + (size_t)s0 * S);

      // level 0: every state; lane l carries states l, l + 64, ...
      unsigned x0[PER0];
#pragma unroll
      for (unsigned j = 0; j < PER0; j++) x0[j] = ((lane + 64u * j) & (size - 1)) * 2u;
      unsigned level = 0, n = size, n1 = 0;
      unsigned w = 0, stop = 1;  // merge points after 4, 16, 48, 128, 512, 2048, 8192, ... symbols
      uint4 cur = gseg[lane];
      auto write_function = [&](unsigned j) {  // F_j[entry of the group] = state here, both as (state - size) * 2
        uint16_t *f = fbuf + (size_t)(fseg[c] + s0 + j) * fstride;
#pragma unroll
        for (unsigned jj = 0; jj < PER0; jj++) {
          const unsigned xi = lane + 64u * jj;
          if (jj < per && xi < size) f[xi] = level == 0 ? (uint16_t)x0[jj] : L.list[L.m[x0[jj]]];
        }
      };
      // behind the prefix: a group down to <= cap classes leaves its candidates to k_seq_candwalk (its later functions are
      // never written); every group's cand0[0] says which way it went
      const bool may_hand = TWO && H.W != 0 && nblk > H.P * sub_blocks;
      bool handed = false;
      auto hand_over = [&]() {
        if (level != 1) return false;
        if (n > H.cap) n = sets_merge<true>(L, n, n1, nw, size, true);
        if (n > H.cap) return false;
        uint16_t *c0 = H.cand0 + (size_t)(fseg[c] + s0) * H.W;
        if (lane < H.W) c0[lane] = L.list[min(lane, n - 1)];
        return true;
      };
      for (unsigned blk = 0; blk < nblk; blk++) {
        // A segment that is S times ONE symbol (a homopolymer context fed its own base) is a power of
        // that symbol's transition: T_s^S from the handle's table, one lookup per carried state instead
        // of S steps -- such a context is (nearly) a permutation of the states, nothing ever merges.
        if (pow != nullptr && blk % sub_blocks == 0) {
          const unsigned s_first = (unsigned)__builtin_amdgcn_readfirstlane(cur.x) & 3u, pat = s_first * 0x01010101u;
          auto differs = [&](const uint4 v) { return (((v.x ^ pat) | (v.y ^ pat) | (v.z ^ pat) | (v.w ^ pat)) & 0x03030303u) != 0u; };
          bool uni = __ballot(differs(cur)) == 0ull;
          for (unsigned b = 1; uni && b < sub_blocks; b++) uni = __ballot(differs(gseg[(size_t)(blk + b) * 64 + lane])) == 0ull;
          if (uni) {
            const char *P = reinterpret_cast<const char *>(pow + (size_t)c * pow_stride + ((size_t)s_first << log));
            if (level == 0) {
#pragma unroll
              for (unsigned j = 0; j < PER0; j++)
                if (j < per) x0[j] = *reinterpret_cast<const uint16_t *>(P + x0[j]);
            } else {
              for (unsigned i = lane; i < n; i += 64) L.list[i] = *reinterpret_cast<const uint16_t *>(P + L.list[i]);
              fq_lds_wave_sync();
            }
            blk += sub_blocks - 1;
            w = (blk + 1) * (SETS_BLOCK / 4);
            while (stop <= w) stop = stop == 1 ? 4 : stop == 4 ? 12 : stop == 12 ? 32 : stop * 4;  // merge points inside the segment are dropped
            if (blk + 1 < nblk) cur = gseg[(size_t)(blk + 1) * 64 + lane];
            write_function(blk / sub_blocks);
            if (may_hand && blk + 1 == H.P * sub_blocks && (handed = hand_over())) break;
            continue;
          }
        }
        const uint4 nxt = blk + 1 < nblk ? gseg[(size_t)(blk + 1) * 64 + lane] : cur;  // lands while cur is walked
        const unsigned wb_end = (blk + 1) * (SETS_BLOCK / 4);
        const uint4 rows = TWO ? sets_pack_rows(cur, log) : cur;
        while (w < wb_end) {
          const unsigned w1 = min(stop, wb_end);
          if (level == 0) {
            for (; w < w1; w++) {
              unsigned row[TWO ? 2 : 4];
              sets_rows<TWO>(sets_word(cur, w), log, row);
#pragma unroll
              for (int i = 0; i < (TWO ? 2 : 4); i++) {
#pragma unroll
                for (unsigned j = 0; j < PER0; j++)
                  if (j < per) x0[j] = *reinterpret_cast<const uint16_t *>(tbase + (row[i] + x0[j]));
              }
            }
          } else {
            switch ((n + 63) / 64) {
              case 1: sets_walk<1, TWO>(L, n, tbase, log, cur, rows, w, w1); break;
              case 2: sets_walk<2, TWO>(L, n, tbase, log, cur, rows, w, w1); break;
              case 3: sets_walk<3, TWO>(L, n, tbase, log, cur, rows, w, w1); break;
              case 4: sets_walk<4, TWO>(L, n, tbase, log, cur, rows, w, w1); break;
              case 5: sets_walk<5, TWO>(L, n, tbase, log, cur, rows, w, w1); break;
              case 6: sets_walk<6, TWO>(L, n, tbase, log, cur, rows, w, w1); break;
              case 7: sets_walk<7, TWO>(L, n, tbase, log, cur, rows, w, w1); break;
              default: sets_walk<8, TWO>(L, n, tbase, log, cur, rows, w, w1); break;
            }
            w = w1;
          }
          if (w != stop || w >= w_end) continue;
          stop = stop == 1 ? 4 : stop == 4 ? 12 : stop == 12 ? 32 : stop * 4;
          if (level == 0) {
            sets_clear(L);
#pragma unroll
            for (unsigned j = 0; j < PER0; j++)
              if (j < per) { const unsigned xi = x0[j] >> 1; atomicOr(&L.bm[xi >> 5], 1u << (xi & 31u)); }
            fq_lds_wave_sync();
            const unsigned nn = sets_count(L, nw);
            if (nn <= SETS_MAX_CLASSES) {  // from here on only the distinct states are carried
#pragma unroll
              for (unsigned j = 0; j < PER0; j++)
                if (j < per) {
                  const unsigned r = sets_rank(L, x0[j] >> 1);
                  L.list[r] = (uint16_t)x0[j];
                  x0[j] = r;  // class of entry state lane + 64 j
                }
              for (unsigned i = lane; i < nn; i += 64) L.m[i] = (uint16_t)i;
              fq_lds_wave_sync();
              level = 1; n = n1 = nn;
            }
          } else if (n > 64) {
            n = sets_merge<true>(L, n, n1, nw, size);
          }
        }
        cur = nxt;
        if ((blk + 1) % sub_blocks == 0) write_function(blk / sub_blocks);
        if (may_hand && blk + 1 == H.P * sub_blocks && (handed = hand_over())) break;
      }
      if (TWO && H.W != 0 && lane == 0) {
        if (!handed) H.cand0[(size_t)(fseg[c] + s0) * H.W] = (uint16_t)SEQ_CAND_KEPT;
        atomicAdd(&H.counts[handed ? 0 : 1], 1u);
      }
      unsigned nk = 0;
      if (lane == 0) nk = atomicAdd(&s_next, 1u);
      k = k0 + (unsigned)__builtin_amdgcn_readfirstlane(nk);
    }
  }
}

// One gather of the candidate walk.  The unit of the walk is a ROW of 16 lanes (a DPP row): the row's lanes hold 16 x 16
// symbols of the row's own segment, unpacked to eight row offsets of the two-symbol table per lane, and lane N's offset
// reaches the whole row as a modifier of the add itself (row_newbcast:N, v_add_u32_dpp): add -> ds_read_u16 -> wait, one
// VALU instruction per gather however many groups share a wave.  (The builtin, not inline assembly: the compiler fuses the
// DPP move into the add and places the wait states a DPP operand needs.)
template <unsigned N>
__device__ __forceinline__ unsigned cand_gather2(unsigned row, unsigned y) {
  const unsigned addr = y + (unsigned)__builtin_amdgcn_update_dpp(0, (int)row, 0x150 + N, 0xF, 0xF, false);
  return *reinterpret_cast<fq_lds_u16 *>((uintptr_t)addr);
}
// the lane's 16 symbols as eight row offsets, one register each
__device__ __forceinline__ void cand_rows(const uint4 cur, unsigned log, unsigned (&r)[8]) {
  const unsigned w[4] = {cur.x, cur.y, cur.z, cur.w};
#pragma unroll
  for (int i = 0; i < 4; i++) {
    r[2 * i] = ((w[i] & 3u) | ((w[i] >> 6) & 0xCu)) << (log + 1);
    r[2 * i + 1] = (((w[i] >> 16) & 3u) | ((w[i] >> 22) & 0xCu)) << (log + 1);
  }
}
// the 256 symbols a row holds: lanes N .. 15 in turn (the DPP control is an immediate, so the 16 lanes are unrolled)
template <unsigned N = 0>
__device__ __forceinline__ unsigned cand_walk256(const unsigned (&r)[8], unsigned y) {
#pragma unroll
  for (int i = 0; i < 8; i++) y = cand_gather2<N>(r[i], y);
  if constexpr (N + 1 < 16) return cand_walk256<N + 1>(r, y);
  else return y;
}

// Step A', two-symbol path: the handed-over groups of one k_seq_setfunc item.  A lane owns (group, candidate k): it starts
// from cand0[group][k], walks segments P .. Q-1 of its group two symbols per gather and stores its state at every segment
// boundary.  A group owns W / 16 rows of 16 lanes, 64 / W groups share a wave (the slots behind a group's n candidates
// shadow the last one, cand0 is padded that way).  Every walked segment is a full S: the chain's last segment belongs to no
// group.  Every row of a group loads the same 16 x 16 bytes of the group's segment per 256 symbols, lane l chunk l (between the
// rows of a group these are hits on the same lines); symbols never pass through LDS.
// LDS: the context's two-symbol table at address 0 and nothing else (64 KB at log 11), so a K3 or K6 workgroup of another
// lane fits beside it.
template <unsigned W>
__global__ void __launch_bounds__(CANDW_WAVES * 64)
k_seq_candwalk(const uint8_t *__restrict__ sorted_sym, const uint32_t *__restrict__ arrays, const uint32_t *__restrict__ plan,
               const uint32_t *__restrict__ logs, const uint16_t *__restrict__ next2, unsigned next_stride, unsigned S,
               unsigned qmax, unsigned gmin, unsigned rounds, const SeqHandover H) {
  static_assert(W == 16 || W == 32 || W == 64, "slots of a wave");
  constexpr unsigned GPW = 64 / W;  // groups per wave
  constexpr unsigned B = SeqModel::B;
  extern __shared__ uint32_t lds[];
  const uint32_t *fitem = plan, *fseg = plan + (B + 1);
  const unsigned item = blockIdx.x;
  if (item >= fitem[B]) return;  // the grid is an upper bound
  const unsigned c = seq_item_ctx(fitem, item);
  const unsigned log = logs[c], size = 1u << log;
  const unsigned nf = fseg[c + 1] - fseg[c], Q = seq_group_of(nf, qmax, gmin), nl = (nf + Q - 1) / Q;
  const unsigned k0 = (item - fitem[c]) * (SETS_WAVES2 * rounds), k_end = min(k0 + SETS_WAVES2 * rounds, nl);
  auto is_handed = [&](unsigned g) { return min(Q, nf - g * Q) > H.P && H.cand0[(size_t)(fseg[c] + g * Q) * W] != SEQ_CAND_KEPT; };
  // (no static LDS, no __syncthreads_or: the table must sit at LDS address 0; the vote goes through its first word)
  if (threadIdx.x == 0) lds[0] = 0;
  __syncthreads();
  for (unsigned g = k0 + threadIdx.x; g < k_end; g += CANDW_WAVES * 64)
    if (is_handed(g)) lds[0] = 1;
  __syncthreads();
  const bool any = lds[0] != 0;
  __syncthreads();
  if (!any) return;  // (uniform) the item kept all its groups: no table to load
  {
    const uint4 *src = reinterpret_cast<const uint4 *>(next2 + (size_t)c * next_stride);
    uint4 *dst = reinterpret_cast<uint4 *>(lds);
    for (unsigned e = threadIdx.x; e < 2 * size; e += CANDW_WAVES * 64) dst[e] = src[e];
  }
  __syncthreads();
  const unsigned wave = threadIdx.x >> 6, lane = fq_lane(), slot = lane / W, kk = lane % W, l = lane & 15u;
  const unsigned chunks = S / 256;  // 16-byte-per-lane loads of a row per segment (S is a multiple of 1024)
  const uint8_t *run = sorted_sym + arrays[B + c];
  for (unsigned ws = wave; k0 + ws * GPW < k_end; ws += CANDW_WAVES) {
    unsigned g = k0 + ws * GPW + slot;
    const bool act = g < k_end && is_handed(g);
    const unsigned long long mask = __ballot(act);
    if (mask == 0ull) continue;  // (wave-uniform)
    // a slot without a handed-over group walks along with the wave's first one and stores nothing
    const unsigned g_first = (unsigned)__builtin_amdgcn_readlane(g, (unsigned)__builtin_amdgcn_readfirstlane((unsigned)__ffsll((long long)mask) - 1u));
    if (!act) g = g_first;
    const unsigned s0 = g * Q, nseg = min(Q, nf - s0);
    unsigned seg_max = 0;  // (wave-uniform) the longest group of the wave; a shorter one repeats its last segment, unstored
#pragma unroll
    for (unsigned t = 0; t < GPW; t++) seg_max = max(seg_max, (unsigned)__builtin_amdgcn_readlane(nseg, t * W));
    const size_t f0 = (size_t)fseg[c] + s0;
    unsigned y = H.cand0[f0 * W + kk];
    auto chunk_at = [&](unsigned j, unsigned ch) {
      return reinterpret_cast<const uint4 *>(run + (size_t)(s0 + min(j, nseg - 1)) * S)[ch * 16 + l];
    };
    uint4 cur = chunk_at(H.P, 0);
    for (unsigned j = H.P; j < seg_max; j++) {
      for (unsigned ch = 0; ch < chunks; ch++) {
        const bool more = ch + 1 < chunks;
        const uint4 nxt = more ? chunk_at(j, ch + 1) : j + 1 < seg_max ? chunk_at(j + 1, 0) : cur;  // lands while cur is walked
        unsigned r[8];
        cand_rows(cur, log, r);
        y = cand_walk256(r, y);
        cur = nxt;
      }
      if (act && j < nseg) H.cand[(f0 + j) * W + kk] = (uint16_t)y;
    }
  }
}

// Step B: entry state of every segment of every chain.  The functions of a group all start at
// the group's entry state, so a group costs one round of independent 2-byte loads, and the chain
// x <- F_last[x] runs from group to group.  A chain of more than SEQ_ITEM_GROUPS groups (one context
// holding most of a block: 3 600 groups for 256 MiB of poly-A) is resolved in three levels over
// ITEMS of 64 groups, like the quality stream's runs of opaque segments:
//  compose  one wave per item: the item's composed function for every possible entry state
//  resolve  one thread per context: item by item
//  expand   one thread per item: group by group inside the item
// The state behind segment j of a group, for the group's entry state e, through ONE set of helpers: a group that kept
// its functions reads F_j[e] from fbuf; a handed-over one has x = F_P[e] (the state behind the prefix) in fbuf, finds the
// candidate k with cand0[group][k] == x (at most W u16 entries, 16 bytes per load; duplicates are harmless) and reads
// cand[j][k].  fg: index of the group's first function.  The HEAD of the group's candidate row (its first 16 bytes) says
// whether the group was handed over and holds the first eight candidates; it depends on nothing but fg, so it is asked for
// together with the group's functions and a kept group still costs ONE round of loads.
constexpr unsigned SEQ_SLOT_KEPT = 0xFFFFFFFFu;
__device__ __forceinline__ uint4 seq_group_head(const SeqHandover &H, size_t fg) {
  return H.W != 0 ? *reinterpret_cast<const uint4 *>(H.cand0 + fg * H.W) : make_uint4(SEQ_CAND_KEPT, 0u, 0u, 0u);
}
__device__ __forceinline__ bool seq_group_handed(const uint4 head) { return (head.x & 0xFFFFu) != SEQ_CAND_KEPT; }
__device__ __forceinline__ unsigned seq_group_slot(const SeqHandover &H, size_t fg, const uint4 head, unsigned x) {
  if (!seq_group_handed(head)) return SEQ_SLOT_KEPT;
  const uint4 *c0 = reinterpret_cast<const uint4 *>(H.cand0 + fg * H.W);
  uint4 v = head;
  for (unsigned i = 0;;) {
    const unsigned w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
    for (unsigned t = 0; t < 8; t++)
      if (((w[t >> 1] >> (16 * (t & 1))) & 0xFFFFu) == x) return 8 * i + t;
    if (++i >= H.W / 8) return 0;  // (not reached: F_P maps into the candidates)
    v = c0[i];
  }
}
__device__ __forceinline__ unsigned seq_state_behind(const SeqHandover &H, const uint16_t *__restrict__ fbuf, unsigned fstride,
                                                     size_t fg, unsigned j, unsigned e, unsigned slot) {
  return slot != SEQ_SLOT_KEPT && j >= H.P ? (unsigned)H.cand[(fg + j) * H.W + slot] : (unsigned)fbuf[(fg + j) * fstride + (e >> 1)];
}

__device__ __forceinline__ unsigned seq_resolve_groups(const uint32_t *__restrict__ fseg, const uint32_t *__restrict__ seg,
                                                       const uint16_t *__restrict__ fbuf, unsigned fstride, unsigned c, unsigned Q,
                                                       unsigned nf, unsigned ns, unsigned s_begin, unsigned s_end, unsigned xo,
                                                       uint16_t *__restrict__ entry, const SeqHandover &H) {
  for (unsigned s0 = s_begin; s0 < s_end; s0 += Q) {
    entry[seg[c] + s0] = (uint16_t)xo;
    const size_t fg = (size_t)fseg[c] + s0;
    const uint4 head = seq_group_head(H, fg);
    unsigned v[SETS_MAX_GROUP];
    // one round of loads from fbuf, the head beside them (behind the prefix of a handed-over group fbuf is stale) ...
#pragma unroll
    for (unsigned j = 0; j < SETS_MAX_GROUP; j++)
      v[j] = j < Q && s0 + j < nf ? seq_state_behind(H, fbuf, fstride, fg, j, xo, SEQ_SLOT_KEPT) : 0u;
    if (seq_group_handed(head) && s0 + H.P < nf && H.P < Q) {  // ... and one from cand, for the candidate that F_P[xo] names
      unsigned xp = 0;
#pragma unroll
      for (unsigned j = 0; j < SETS_MAX_GROUP; j++) xp = j + 1 == H.P ? v[j] : xp;
      const unsigned slot = seq_group_slot(H, fg, head, xp);
#pragma unroll
      for (unsigned j = 0; j < SETS_MAX_GROUP; j++)
        if (j >= H.P && j < Q && s0 + j < nf) v[j] = seq_state_behind(H, fbuf, fstride, fg, j, xo, slot);
    }
    unsigned nx = xo;
#pragma unroll
    for (unsigned j = 0; j < SETS_MAX_GROUP; j++)
      if (j < Q && s0 + j < nf) {
        if (j + 1 < Q) entry[seg[c] + s0 + j + 1] = (uint16_t)v[j]; else nx = v[j];
      }
    xo = nx;
  }
  (void)ns;
  return xo;
}

constexpr unsigned SEQ_RESOLVE_THREADS = 1024;

// the composed function of one item (64 groups) for every possible entry state; one wave
template <unsigned PER0>
__device__ __forceinline__ void seq_compose_item(const uint32_t *__restrict__ plan, const uint32_t *__restrict__ logs,
                                                 const uint16_t *__restrict__ fbuf, unsigned fstride, unsigned qmax, unsigned gmin,
                                                 unsigned item, uint16_t *__restrict__ cbuf, const SeqHandover &H) {
  constexpr unsigned B = SeqModel::B;
  const uint32_t *fseg = plan + (B + 1), *citem = plan + 4 * (B + 1);
  const unsigned lane = fq_lane();
  const unsigned c = seq_item_ctx(citem, item);
  const unsigned nf = fseg[c + 1] - fseg[c], Q = seq_group_of(nf, qmax, gmin), nl = (nf + Q - 1) / Q;
  const unsigned g0 = (item - citem[c]) * SEQ_ITEM_GROUPS, g1 = min(g0 + SEQ_ITEM_GROUPS, nl);
  const unsigned size = 1u << logs[c], per = max(size >> 6, 1u);
  unsigned x[PER0];  // (state - size) * 2 behind the groups walked so far, for every entry state of the item
#pragma unroll
  for (unsigned j = 0; j < PER0; j++) x[j] = ((lane + 64u * j) & (size - 1)) * 2u;
  // which of the item's groups were handed over: lane l asks for group g0 + l, before the chain through the groups starts
  const unsigned long long handed = __ballot(g0 + lane < g1 && seq_group_handed(seq_group_head(H, (size_t)fseg[c] + (g0 + lane) * Q)));
  for (unsigned g = g0; g < g1; g++) {
    const unsigned last = min(Q, nf - g * Q) - 1;  // the group's last function: entry of the group -> entry of the next
    const size_t fg = (size_t)fseg[c] + g * Q;
    if (((handed >> (g - g0)) & 1ull) == 0ull) {  // (wave-uniform)
#pragma unroll
      for (unsigned j = 0; j < PER0; j++)
        if (j < per) x[j] = seq_state_behind(H, fbuf, fstride, fg, last, x[j], SEQ_SLOT_KEPT);
    } else {  // three rounds: the state behind the prefix, its candidate, the candidate's state behind the group
      const uint4 head = seq_group_head(H, fg);
#pragma unroll
      for (unsigned j = 0; j < PER0; j++)
        if (j < per) x[j] = seq_state_behind(H, fbuf, fstride, fg, H.P - 1, x[j], SEQ_SLOT_KEPT);
#pragma unroll
      for (unsigned j = 0; j < PER0; j++)
        if (j < per) x[j] = seq_group_slot(H, fg, head, x[j]);
#pragma unroll
      for (unsigned j = 0; j < PER0; j++)
        if (j < per) x[j] = seq_state_behind(H, fbuf, fstride, fg, last, 0u, x[j]);
    }
  }
  uint16_t *o = cbuf + (size_t)item * fstride;
#pragma unroll
  for (unsigned j = 0; j < PER0; j++) {
    const unsigned xi = lane + 64u * j;
    if (j < per && xi < size) o[xi] = (uint16_t)x[j];
  }
}

// One workgroup, one launch (every kernel boundary on a lane's stream is a wait for the chip to have
// room again): thread c resolves a short chain group by group; long chains go through the three
// levels, the levels separated by workgroup barriers.
template <unsigned PER0>
__global__ void __launch_bounds__(SEQ_RESOLVE_THREADS)
k_seq_resolve(const uint32_t *__restrict__ plan, const uint32_t *__restrict__ logs, const uint16_t *__restrict__ fbuf,
              unsigned fstride, unsigned qmax, unsigned gmin, uint16_t *__restrict__ cbuf, uint16_t *__restrict__ item_entry,
              uint16_t *__restrict__ entry, const SeqHandover H) {
  constexpr unsigned B = SeqModel::B;
  const uint32_t *fseg = plan + (B + 1), *seg = plan + 2 * (B + 1), *citem = plan + 4 * (B + 1);
  const unsigned c = threadIdx.x;
  unsigned ns = 0, nf = 0, Q = 1, ni = 0;
  if (c < B) {
    ns = seg[c + 1] - seg[c]; nf = ns ? ns - 1 : 0; Q = seq_group_of(nf, qmax, gmin);
    ni = citem[c + 1] - citem[c];
    if (ni == 0) (void)seq_resolve_groups(fseg, seg, fbuf, fstride, c, Q, nf, ns, 0, ns, 0u, entry, H);  // FSE_initCState: state = size
  }
  const unsigned n_items = citem[B];
  if (n_items == 0) return;  // (uniform) no long chain in this block
  for (unsigned item = threadIdx.x >> 6; item < n_items; item += SEQ_RESOLVE_THREADS / 64)
    seq_compose_item<PER0>(plan, logs, fbuf, fstride, qmax, gmin, item, cbuf, H);
  __threadfence();
  __syncthreads();
  if (c < B && ni) {
    unsigned xo = 0;
    for (unsigned i = 0; i < ni; i++) {
      item_entry[citem[c] + i] = (uint16_t)xo;
      if (i + 1 < ni) xo = __hip_atomic_load(&cbuf[(size_t)(citem[c] + i) * fstride + (xo >> 1)], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
  }
  __threadfence();
  __syncthreads();
  for (unsigned item = threadIdx.x; item < n_items; item += SEQ_RESOLVE_THREADS) {
    const unsigned ic = seq_item_ctx(citem, item);
    const unsigned ins = seg[ic + 1] - seg[ic], inf = ins ? ins - 1 : 0, iQ = seq_group_of(inf, qmax, gmin);
    // (the chain's LAST segment has no function of its own and belongs to no group: when the functions fill the
    // last item's 64 groups exactly, s_begin + 64 * iQ stops one segment short of it -- the last item runs to the end)
    const unsigned s_begin = (item - citem[ic]) * SEQ_ITEM_GROUPS * iQ;
    const unsigned s_end = item + 1 == citem[ic + 1] ? ins : min(s_begin + SEQ_ITEM_GROUPS * iQ, ins);
    const unsigned xo = __hip_atomic_load(&item_entry[item], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    (void)seq_resolve_groups(fseg, seg, fbuf, fstride, ic, iQ, inf, ins, s_begin, s_end, xo, entry, H);
  }
}

// Step C: one lane per segment, 64 segments of one context per wave.  The chain of a lane is short (state -> one
// ds_read_u16 of next1[s][x] -> state), but a lone wave issues one instruction per four cycles, so every instruction of
// the step is on the clock.  The loop therefore works in ROUNDS of 64 symbols:
//  - the 64 symbols of the next round (four 16-byte loads) are asked for in front of the walk and waited for behind it;
//  - a symbol's deltaNbBits is picked with two bit tests (three selects, no branch);
//  - the round's 128 bytes of out16 are one cache line and leave with eight stores in a row, which this loop never waits
//    for: gfx9 counts loads and stores in one counter, the next symbols were asked for in front of the stores, so the
//    wait for them (vmcnt(8)) leaves the stores in flight -- provided nothing else is pending when the loop is entered.
// What a whole round does not cover, the end of a chain's last segment, goes in groups of 16 with the state frozen
// behind the chain's last symbol (one group asked for ahead, and a wait for everything per group, as before).
// (Splitting the walk -- one wave walks the states alone and notes them every 512 symbols, eight waves emit the pieces --
// makes the kernel shorter alone and the step slower: DESIGN.md section 8.)

// one step of the state chain: state (as (state - size) * 2) behind symbol s
__device__ __forceinline__ unsigned emit_next(const char *tbase, unsigned log1, unsigned s, unsigned xo) {
  return *reinterpret_cast<const uint16_t *>(tbase + ((s << log1) + xo));
}

__global__ void __launch_bounds__(64)
k_seq_emit(const uint8_t *__restrict__ sorted_sym, uint16_t *__restrict__ out16,
           const uint32_t *__restrict__ arrays, const uint32_t *__restrict__ plan,
           const uint32_t *__restrict__ ct, const uint32_t *__restrict__ ct_off,
           const uint16_t *__restrict__ next1, unsigned next_stride, unsigned S,
           const uint16_t *__restrict__ entry, uint16_t *__restrict__ final_state, StreamResult *res) {
  extern __shared__ uint32_t lds[];
  constexpr unsigned B = SeqModel::B;
  const uint32_t *seg = plan + 2 * (B + 1), *eitem = plan + 3 * (B + 1);
  if (blockIdx.x >= eitem[B]) return;  // the grid is an upper bound
  const unsigned c = seq_item_ctx(eitem, blockIdx.x);
  const uint32_t *tbl = ct + ct_off[c];
  const unsigned log = tbl[0] & 0xFFFFu, size = 1u << log, log1 = log + 1;
  {
    const uint4 *src = reinterpret_cast<const uint4 *>(next1 + (size_t)c * next_stride);
    uint4 *dst = reinterpret_cast<uint4 *>(lds);
    for (unsigned e = threadIdx.x; e < size / 2; e += 64) dst[e] = src[e];
  }
  const uint32_t *tt = tbl + 1 + (size >> 1);
  unsigned dnb[4];
#pragma unroll
  for (int s = 0; s < 4; s++) dnb[s] = tt[2 * s + 1];
  fq_lds_wave_sync();
  const unsigned n = arrays[c], ns = seg[c + 1] - seg[c];
  const unsigned k = (blockIdx.x - eitem[c]) * 64 + fq_lane();
  if (k >= ns) return;
  const char *tbase = reinterpret_cast<const char *>(lds);
  const size_t run0 = (size_t)arrays[B + c] + (size_t)k * S;  // 16-byte aligned
  const unsigned len = min(S, n - k * S);
  const uint4 *gsym = reinterpret_cast<const uint4 *>(sorted_sym + run0);
  uint4 *gout = reinterpret_cast<uint4 *>(out16 + run0);
  unsigned xo = entry[seg[c] + k];
  auto packed = [&](unsigned s) {  // (nb << 12 | bits) of symbol s in state xo
    const unsigned x = size + (xo >> 1);
    const unsigned d01 = (s & 1u) ? dnb[1] : dnb[0], d23 = (s & 1u) ? dnb[3] : dnb[2];
    const unsigned nb = (x + ((s & 2u) ? d23 : d01)) >> 16;
    return (nb << 12) | (x & ((1u << nb) - 1u));
  };
  const unsigned full = len >> 6, last = full ? full - 1 : 0u;  // whole rounds
  uint4 sv[4], nv[4];
#pragma unroll
  for (int q = 0; q < 4; q++) sv[q] = gsym[q];  // (a run of fewer than 64 symbols: still inside the buffer, EncShape::padded)
  // The first symbols and the entry state are USED here (empty statements that take them as operands), so they have arrived and nothing is
  // in flight when the loop is entered: inside it the only wait for memory is then the one behind the stores, for the
  // next round's symbols, which were asked for in front of the stores and leaves them in flight.
#pragma unroll
  for (int q = 0; q < 4; q++) asm volatile("" : "+v"(sv[q].x), "+v"(sv[q].y), "+v"(sv[q].z), "+v"(sv[q].w));
  asm volatile("" : "+v"(xo));  // (the entry state as well: it was asked for behind them)
  for (unsigned ch = 0; ch < full; ch++) {
    const uint4 *nx = gsym + 4 * min(ch + 1, last);
#pragma unroll
    for (int q = 0; q < 4; q++) nv[q] = nx[q];
    __builtin_amdgcn_sched_barrier(0);  // (the loads stay in front of the walk that hides them ...)
    unsigned o[32];
#pragma unroll
    for (int q = 0; q < 4; q++) {
      const unsigned wds[4] = {sv[q].x, sv[q].y, sv[q].z, sv[q].w};
#pragma unroll
      for (int j = 0; j < 16; j++) {
        const unsigned s = (wds[j >> 2] >> (8 * (j & 3))) & 3u, v = packed(s);
        if (j & 1) o[8 * q + (j >> 1)] |= v << 16; else o[8 * q + (j >> 1)] = v;
        xo = emit_next(tbase, log1, s, xo);
      }
    }
    __builtin_amdgcn_sched_barrier(0);  // (... the stores stay together ...)
#pragma unroll
    for (int q = 0; q < 8; q++) gout[8 * ch + q] = make_uint4(o[4 * q], o[4 * q + 1], o[4 * q + 2], o[4 * q + 3]);
    __builtin_amdgcn_sched_barrier(0);  // (... and the loads are waited for behind them)
#pragma unroll
    for (int q = 0; q < 4; q++) sv[q] = nv[q];
  }
  // the end of a chain's last segment, in groups of 16, the next group's symbols asked for a group ahead: the run is
  // padded to 16, the pad is walked and never read back
  const unsigned groups = (len + 15) >> 4;
  if (full * 4 < groups) {
    uint4 tv = gsym[full * 4];
    for (unsigned g = full * 4; g < groups; g++) {
      const uint4 tv_next = gsym[g + 1 < groups ? g + 1 : g];
      const unsigned wds[4] = {tv.x, tv.y, tv.z, tv.w};
      const unsigned live = min(16u, len - g * 16);
      unsigned o[8];
#pragma unroll
      for (int j = 0; j < 16; j++) {
        const unsigned s = (wds[j >> 2] >> (8 * (j & 3))) & 3u, v = packed(s);
        if (j & 1) o[j >> 1] |= v << 16; else o[j >> 1] = v;
        const unsigned nxs = emit_next(tbase, log1, s, xo);
        if ((unsigned)j < live) xo = nxs;  // the state stops at the end of the chain
      }
      gout[2 * g] = make_uint4(o[0], o[1], o[2], o[3]);
      gout[2 * g + 1] = make_uint4(o[4], o[5], o[6], o[7]);
      tv = tv_next;
    }
  }
  if (k == ns - 1) final_state[c] = (uint16_t)(size + (xo >> 1));
  if (fq_lane() == 0) atomicMax(&res->refixed, len);
}
