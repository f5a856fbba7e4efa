// graphbuild.hip -- the kernels around the ordered rounds that only stream: graph construction of a stage (links, instance lists in the
// reference's initial order, E2), the block index of the original slots, and the copy-back (T3, reference src/blockfinder.cpp:85-95).
#include <cstring>
#include <algorithm>
#include <vector>
#include "simplify_device.h"

// ------------------------------------------------------------------------------------------- graph construction kernels
__global__ void __launch_bounds__(256) k_init_links(unsigned *__restrict__ nx, unsigned *__restrict__ pv, unsigned *__restrict__ nodeof0,
                                                    unsigned *__restrict__ nodeof1, uint8_t *__restrict__ ch, size_t E, size_t cap)
{
	size_t e = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
	if (e >= cap) return;
	if (e < E) { nx[e] = e + 1 < E ? (unsigned)(e + 1) : SBL_NONE; pv[e] = e ? (unsigned)(e - 1) : SBL_NONE; }
	else { nx[e] = pv[e] = SBL_NONE; ch[e] = BT_DEAD_CHAR; }
	nodeof0[e] = nodeof1[e] = SBL_NONE;
}

// ---- marks of both strands and the block index of a stage start: ONE pass over bif[0], bif[1] and ch of the original slots ----------
// A wave takes MARK_CHUNK = 256 consecutive slots, four per lane (16-byte loads), i.e. four blocks of the block index.  The ballot of
// "element j of my four" has one bit per lane; spread4 moves the 16 lanes of a block to every fourth bit, so the four ballots interleave
// into the block's 64-bit mask.  Per wave: the counts of both strands' marks (cnt[wave], cnt[nchunks + wave]; their exclusive scan gives
// k_write_marks2 its offsets and, at [nchunks] and [2 nchunks], the totals) and -- bidx != nullptr -- the four index records: marks
// of strand 0, of strand 1, separators, and word 3 = 0 (at a stage start every block is pristine and unstamped: k_build_blkidx).
__device__ __forceinline__ unsigned long long spread4(unsigned long long x)      // bit i of the low 16 -> bit 4 i
{
	unsigned long long v = x & 0xFFFFull;
	v = (v | (v << 24)) & 0x000000FF000000FFull;
	v = (v | (v << 12)) & 0x000F000F000F000Full;
	v = (v | (v << 6)) & 0x0303030303030303ull;
	v = (v | (v << 3)) & 0x1111111111111111ull;
	return v;
}
__device__ __forceinline__ void load4(const unsigned *__restrict__ a, size_t e0, size_t E, unsigned (&v)[4])
{
	if (e0 + 4 <= E) { const uint4 q = *reinterpret_cast<const uint4 *>(a + e0); v[0] = q.x; v[1] = q.y; v[2] = q.z; v[3] = q.w; }
	else for (int j = 0; j < 4; j++) v[j] = e0 + j < E ? a[e0 + j] : SBL_NONE;
}
__global__ void __launch_bounds__(256) k_count_marks2(const unsigned *__restrict__ bif0, const unsigned *__restrict__ bif1, const uint8_t *__restrict__ ch, size_t E,
                                                      unsigned nchunks, unsigned *__restrict__ cnt, unsigned long long *__restrict__ bidx)
{
	const unsigned wave = blockIdx.x * 4u + (threadIdx.x >> 6), lane = threadIdx.x & 63u;
	if (wave >= nchunks) return;                    // (wave-uniform)
	const size_t e0 = (size_t)wave * MARK_CHUNK + lane * 4u;
	unsigned a[4], b[4], s[4];
	load4(bif0, e0, E, a); load4(bif1, e0, E, b);
	if (e0 + 4 <= E) { const unsigned q = *reinterpret_cast<const unsigned *>(ch + e0); for (int j = 0; j < 4; j++) s[j] = (q >> (8 * j)) & 0xFFu; }
	else for (int j = 0; j < 4; j++) s[j] = e0 + j < E ? ch[e0 + j] : 0u;
	unsigned long long m0[4], m1[4], sp[4];
	unsigned n0 = 0, n1 = 0;
#pragma unroll
	for (int j = 0; j < 4; j++) {
		m0[j] = __ballot(a[j] != SBL_NONE); m1[j] = __ballot(b[j] != SBL_NONE); sp[j] = __ballot(s[j] == BT_SEP);
		n0 += (unsigned)__popcll(m0[j]); n1 += (unsigned)__popcll(m1[j]);
	}
	if (lane == 0) { cnt[wave] = n0; cnt[nchunks + wave] = n1; }
	const size_t blk = (size_t)wave * 4u + lane;    // lanes 0 .. 3: one block of 64 slots each
	if (bidx && lane < 4u && blk * 64u < E) {
		const unsigned sh = 16u * lane;
		unsigned long long w0 = 0, w1 = 0, w2 = 0;
#pragma unroll
		for (int j = 0; j < 4; j++) { w0 |= spread4(m0[j] >> sh) << j; w1 |= spread4(m1[j] >> sh) << j; w2 |= spread4(sp[j] >> sh) << j; }
		unsigned long long *w = bidx + blk * BT_IDX_WORDS;
		w[0] = w0; w[1] = w1; w[2] = w2; w[3] = 0ull;
	}
}
// ordered compaction of both strands' marks into (element, id) arrays; off = exclusive scan of k_count_marks2's counts
__global__ void __launch_bounds__(256) k_write_marks2(const unsigned *__restrict__ bif0, const unsigned *__restrict__ bif1, size_t E, unsigned nchunks,
                                                      const unsigned *__restrict__ off, unsigned *__restrict__ melem0, unsigned *__restrict__ mid0,
                                                      unsigned *__restrict__ melem1, unsigned *__restrict__ mid1)
{
	const unsigned wave = blockIdx.x * 4u + (threadIdx.x >> 6), lane = threadIdx.x & 63u;
	if (wave >= nchunks) return;                    // (wave-uniform)
	const size_t e0 = (size_t)wave * MARK_CHUNK + lane * 4u;
	const unsigned total0 = off[nchunks];
#pragma unroll
	for (int t = 0; t < 2; t++) {
		unsigned ids[4], n = 0;
		load4(t ? bif1 : bif0, e0, E, ids);
		for (int j = 0; j < 4; j++) n += ids[j] != SBL_NONE;
		unsigned incl = n;
#pragma unroll
		for (int d = 1; d < 64; d <<= 1) { const unsigned v = __shfl_up(incl, d); if (lane >= (unsigned)d) incl += v; }
		unsigned o = off[t * nchunks + wave] - (t ? total0 : 0u) + incl - n;
		unsigned *__restrict__ oe = t ? melem1 : melem0, *__restrict__ oi = t ? mid1 : mid0;
		for (int j = 0; j < 4; j++) if (ids[j] != SBL_NONE) { oe[o] = (unsigned)(e0 + j); oi[o] = ids[j]; o++; }
	}
}

// The initial slist order of BifurcationStorage (front insertion while scanning (chr,pos) ascending, reference
// src/indexedsequence.cpp:51-67 + src/bifurcationstorage.cpp:122): + list = elements descending; - list = chromosomes descending,
// elements ascending.  The compact mark arrays (ascending element per strand) already hold that order up to a permutation that needs no
// sort: strand 0 reversed; strand 1 chromosome by chromosome from the last, which the marks before each separator give (lb[c] = marks
// of strand 1 that lie before chromosome c, lb[nchr] = all of them).  k_instance_input places every mark at that rank in ONE array for
// both strands, with the key (strand << idbits) | id; a STABLE sort over the idbits + 1 key bits then leaves (strand, id, order):
// sorted position = node number.
__global__ void __launch_bounds__(64) k_mark_bounds(const unsigned *__restrict__ melem1, unsigned n1, const unsigned *__restrict__ sepidx, unsigned nchr, unsigned *__restrict__ lb)
{
	const unsigned c = blockIdx.x * blockDim.x + threadIdx.x;
	if (c > nchr) return;
	unsigned lo = 0, hi = c == 0 ? 0u : n1;             // marks with element <= sepidx[c]: what chr_of puts into the chromosomes before c
	if (c == nchr) lo = n1;
	const unsigned sep = sepidx[c];
	while (lo < hi) { const unsigned mid = (lo + hi) >> 1; if (melem1[mid] <= sep) lo = mid + 1; else hi = mid; }
	lb[c] = lo;
}
// ... and, as it has the element and its chromosome in hand, the endChar bit and the distance to the chromosome end of every mark
// (aux, what the first snapshot's stream reads per mark: snapshot.hip, k_snapshot_first)
__global__ void __launch_bounds__(256) k_instance_input(const unsigned *__restrict__ melem0, const unsigned *__restrict__ mid0, const unsigned *__restrict__ melem1,
                                                        const unsigned *__restrict__ mid1, unsigned n0, unsigned n1, const unsigned *__restrict__ sepidx, unsigned nchr,
                                                        const unsigned *__restrict__ lb, const uint8_t *__restrict__ ch, unsigned k, unsigned idbits,
                                                        unsigned *__restrict__ keys, unsigned *__restrict__ midx, unsigned *__restrict__ aux0, unsigned *__restrict__ aux1)
{
	const unsigned i = blockIdx.x * blockDim.x + threadIdx.x;
	if (i >= n0 + n1) return;
	const unsigned strand = i >= n0 ? 1u : 0u, j = strand ? i - n0 : i;
	const unsigned e = strand ? melem1[j] : melem0[j], id = strand ? mid1[j] : mid0[j], c = chr_of(sepidx, nchr, e);
	const unsigned p = strand ? n0 + (n1 - lb[c + 1]) + (j - lb[c]) : n0 - 1u - j;
	keys[p] = (strand << idbits) | id;
	midx[p] = j;                                    // payload of the sort: index into the strand's positional (compact) mark arrays
	const unsigned dist = strand == 0 ? sepidx[c + 1] - e : e - sepidx[c];      // valid steps from the instance (inclusive) to the separator
	unsigned bit = 0;
	if (dist >= k + 1) {                                                         // ProperKMer(k + 1): endChar = character at step k, oriented
		const uint8_t x = strand == 0 ? ch[e + k] : ch[e - k];
		const unsigned code = x == 'A' ? 0u : x == 'C' ? 1u : x == 'G' ? 2u : 3u;
		bit = 1u << (strand == 0 ? code : 3u - code);
	}
	(strand ? aux1 : aux0)[j] = (bit << 24) | (dist < 0xFFFFFFu ? dist : 0xFFFFFFu);
}

__global__ void __launch_bounds__(256) k_build_lists(const unsigned *__restrict__ skeys, const unsigned *__restrict__ smidx, const unsigned *__restrict__ melem0,
                                                     const unsigned *__restrict__ melem1, unsigned n, unsigned idbits, unsigned *__restrict__ nslot, unsigned *__restrict__ nnext,
                                                     unsigned *__restrict__ nidst, uint8_t *__restrict__ ndead, unsigned *__restrict__ head0, unsigned *__restrict__ head1,
                                                     unsigned *__restrict__ lsize0, unsigned *__restrict__ lsize1, unsigned *__restrict__ nodeof0, unsigned *__restrict__ nodeof1,
                                                     unsigned *__restrict__ nmark)
{
	const unsigned nd = blockIdx.x * blockDim.x + threadIdx.x;
	if (nd >= n) return;
	const unsigned key = skeys[nd], j = smidx[nd];
	const unsigned strand = key >> idbits, id = key & ((1u << idbits) - 1u), e = strand ? melem1[j] : melem0[j];
	nmark[nd] = j;                                  // where the instance sits in the positional mark arrays (k_snapshot_first)
	const bool last = nd + 1 >= n || skeys[nd + 1] != key;
	const bool first = nd == 0 || skeys[nd - 1] != key;
	nslot[nd] = e; ndead[nd] = 0; nidst[nd] = (id << 1) | strand;
	nnext[nd] = last ? SBL_NONE : nd + 1;
	(strand ? nodeof1 : nodeof0)[e] = nd;
	if (first) {
		// the list's size = the length of its run in the sorted array (an atomic per instance kept this kernel in issue stalls for two
		// thirds of its time: SQ_WAIT_INST_ANY 66 %, profiles/r03_sq_counters.json)
		(strand ? head1 : head0)[id] = nd;
		unsigned len = 1;
		while (nd + len < n && skeys[nd + len] == key) len++;
		(strand ? lsize1 : lsize0)[id] = len;
	}
}

// largest number of instances of any id (sizes the per-transaction scratch arena)
// Snapshot order: ids sorted by where (one of) their instances lies, so that the workgroups resident at the same time scan
// overlapping windows (an element is covered by ~17 windows at 8 strains) and meet in L2 instead of re-reading HBM.
__global__ void __launch_bounds__(256) k_id_position_keys(const unsigned *__restrict__ head0, const unsigned *__restrict__ head1, const unsigned *__restrict__ nslot,
                                                          unsigned nid, unsigned long long *__restrict__ keys, unsigned *__restrict__ ids)
{
	unsigned id = blockIdx.x * blockDim.x + threadIdx.x;
	if (id >= nid) return;
	unsigned nd = head0[id] != BT_NONE ? head0[id] : head1[id];
	keys[id] = nd != BT_NONE ? nslot[nd] : 0xFFFFFFFFull;
	ids[id] = id;
}

__global__ void __launch_bounds__(256) k_max_instances(const unsigned *__restrict__ l0, const unsigned *__restrict__ l1, unsigned nid, unsigned *__restrict__ out)
{
	unsigned m = 0;
	for (unsigned i = blockIdx.x * blockDim.x + threadIdx.x; i < nid; i += gridDim.x * blockDim.x) { unsigned v = l0[i] + l1[i]; m = v > m ? v : m; }
	for (int d = 32; d > 0; d >>= 1) { unsigned v = __shfl_down(m, d); m = v > m ? v : m; }
	if ((threadIdx.x & 63) == 0) atomicMax(out, m);
}

// ------------------------------------------------------------------------------------------- copy-back (T3) kernels
// The list is a chain of "segments" = maximal runs of consecutive slots linked consecutively.  Heads are
// found with a flag pass, segments are ranked by pointer jumping, elements scatter to rank + offset.
// The head flags are kept as one 64-bit mask per 64 slots (a wave's ballot) with its popcount; segoff = exclusive scan of the popcounts
// over the ne / 64 blocks, and the segment of a live element is seg_of(): the heads before its block plus those up to it in the block.
__device__ __forceinline__ unsigned seg_of(const unsigned long long *__restrict__ segmask, const unsigned *__restrict__ segoff, unsigned e)
{
	const unsigned b = e >> 6;
	return segoff[b] + (unsigned)__popcll(segmask[b] & (~0ull >> (63u - (e & 63u)))) - 1u;
}
__global__ void __launch_bounds__(256) k_seg_flags(const uint8_t *__restrict__ ch, const unsigned *__restrict__ nx, unsigned ne, unsigned long long *__restrict__ segmask,
                                                   unsigned *__restrict__ segcnt)
{
	// a wave takes MARK_CHUNK slots, four per lane (16-byte loads of nx), as k_count_marks2 does; link(e) = e is alive and its link
	// points at e + 1, and e is a head iff it is alive and link(e - 1) does not hold
	const unsigned wave = blockIdx.x * 4u + (threadIdx.x >> 6), lane = threadIdx.x & 63u;
	if (wave >= (ne + MARK_CHUNK - 1u) / MARK_CHUNK) return;      // (wave-uniform)
	const size_t e0 = (size_t)wave * MARK_CHUNK + lane * 4u;
	unsigned n[4], c[4];
	load4(nx, e0, ne, n);
	if (e0 + 4 <= ne) { const unsigned q = *reinterpret_cast<const unsigned *>(ch + e0); for (int j = 0; j < 4; j++) c[j] = (q >> (8 * j)) & 0xFFu; }
	else for (int j = 0; j < 4; j++) c[j] = e0 + j < ne ? ch[e0 + j] : (unsigned)BT_DEAD_CHAR;
	int alive[4], link[4];
#pragma unroll
	for (int j = 0; j < 4; j++) { alive[j] = c[j] != (unsigned)BT_DEAD_CHAR; link[j] = alive[j] && n[j] == (unsigned)(e0 + j + 1); }
	int before = __shfl_up(link[3], 1);                           // link(e0 - 1): the lane below has it, lane 0 reads it
	if (lane == 0) before = e0 > 0 && ch[e0 - 1] != BT_DEAD_CHAR && nx[e0 - 1] == (unsigned)e0;
	unsigned long long hb[4];
#pragma unroll
	for (int j = 0; j < 4; j++) hb[j] = __ballot(alive[j] && !(j ? link[j - 1] : before));
	const size_t blk = (size_t)wave * 4u + lane;                  // lanes 0 .. 3: one block of 64 slots each
	if (lane < 4u && blk * 64u < ne) {
		unsigned long long m = 0;
#pragma unroll
		for (int j = 0; j < 4; j++) m |= spread4(hb[j] >> (16u * lane)) << j;
		segmask[blk] = m; segcnt[blk] = (unsigned)__popcll(m);
	}
}
// For every alive head / tail element: record its segment's head, tail and successor.
__global__ void __launch_bounds__(256) k_seg_tails(const uint8_t *__restrict__ ch, const unsigned *__restrict__ nx, unsigned ne,
                                                   const unsigned long long *__restrict__ segmask, const unsigned *__restrict__ segoff /* exclusive scan */,
                                                   unsigned *__restrict__ seg_head, unsigned *__restrict__ seg_len, unsigned *__restrict__ seg_succ_elem)
{
	unsigned e = blockIdx.x * blockDim.x + threadIdx.x;
	if (e >= ne || ch[e] == BT_DEAD_CHAR) return;
	const bool head = (segmask[e >> 6] >> (e & 63u)) & 1ull;
	const bool tail = !(e + 1 < ne && ch[e + 1] != BT_DEAD_CHAR && nx[e] == e + 1);
	if (!head && !tail) return;
	const unsigned seg = seg_of(segmask, segoff, e);
	if (head) seg_head[seg] = e;
	if (tail) { seg_len[seg] = e; seg_succ_elem[seg] = nx[e]; }   // seg_len temporarily holds the tail element
}
__global__ void __launch_bounds__(256) k_seg_finish(unsigned nseg, const unsigned *__restrict__ seg_head, unsigned *__restrict__ seg_len,
                                                    const unsigned *__restrict__ seg_succ_elem, const unsigned long long *__restrict__ segmask,
                                                    const unsigned *__restrict__ segoff, unsigned *__restrict__ succ, unsigned long long *__restrict__ dist)
{
	unsigned s = blockIdx.x * blockDim.x + threadIdx.x;
	if (s >= nseg) return;
	unsigned len = seg_len[s] - seg_head[s] + 1;
	seg_len[s] = len;
	unsigned se = seg_succ_elem[s];
	succ[s] = se == SBL_NONE ? SBL_NONE : seg_of(segmask, segoff, se);
	dist[s] = len;
}
// Wyllie pointer jumping: dist[s] = total length from s to the end of the chain
__global__ void __launch_bounds__(256) k_seg_jump(unsigned nseg, const unsigned *__restrict__ succ_in, const unsigned long long *__restrict__ dist_in,
                                                  unsigned *__restrict__ succ_out, unsigned long long *__restrict__ dist_out)
{
	unsigned s = blockIdx.x * blockDim.x + threadIdx.x;
	if (s >= nseg) return;
	unsigned n = succ_in[s];
	if (n == SBL_NONE) { succ_out[s] = SBL_NONE; dist_out[s] = dist_in[s]; }
	else { succ_out[s] = succ_in[n]; dist_out[s] = dist_in[s] + dist_in[n]; }
}
__global__ void __launch_bounds__(256) k_scatter_linear(const uint8_t *__restrict__ ch, const unsigned *__restrict__ op, unsigned ne,
                                                        const unsigned long long *__restrict__ segmask, const unsigned *__restrict__ segoff,
                                                        const unsigned *__restrict__ seg_head, const unsigned long long *__restrict__ dist,
                                                        unsigned long long total, uint8_t *__restrict__ ch_out, unsigned *__restrict__ op_out,
                                                        unsigned *__restrict__ newidx /* nullptr: nobody reads the full map (k_dict_check does) */)
{
	unsigned e = blockIdx.x * blockDim.x + threadIdx.x;
	if (e >= ne) return;
	if (ch[e] == BT_DEAD_CHAR) { if (newidx) newidx[e] = SBL_NONE; return; }
	unsigned seg = seg_of(segmask, segoff, e);
	unsigned long long pos = total - dist[seg] + (e - seg_head[seg]);
	ch_out[pos] = ch[e];
	op_out[pos] = op[e] & BT_POS_MASK;
	if (newidx) newidx[e] = (unsigned)pos;
}
// the separators' new slots, straight from the ranking (they are live elements of the final list)
__global__ void k_remap_seps(const unsigned long long *__restrict__ segmask, const unsigned *__restrict__ segoff, const unsigned *__restrict__ seg_head,
                             const unsigned long long *__restrict__ dist, unsigned long long total, unsigned *__restrict__ sepidx, unsigned n)
{
	unsigned i = blockIdx.x * blockDim.x + threadIdx.x;
	if (i >= n) return;
	const unsigned e = sepidx[i], seg = seg_of(segmask, segoff, e);
	sepidx[i] = (unsigned)(total - dist[seg] + (e - seg_head[seg]));
}
// list position of every live element and its inverse (the linearised marks of the later snapshots, snapshot.hip)
__global__ void __launch_bounds__(256) k_lin_positions(const uint8_t *__restrict__ ch, unsigned ne, const unsigned long long *__restrict__ segmask, const unsigned *__restrict__ segoff,
                                                       const unsigned *__restrict__ seg_head, const unsigned long long *__restrict__ dist, unsigned long long total,
                                                       unsigned *__restrict__ lin, unsigned *__restrict__ elin)
{
	unsigned e = blockIdx.x * blockDim.x + threadIdx.x;
	if (e >= ne) return;
	if (ch[e] == BT_DEAD_CHAR) { lin[e] = SBL_NONE; return; }
	unsigned seg = seg_of(segmask, segoff, e);
	unsigned pos = (unsigned)(total - dist[seg] + (e - seg_head[seg]));
	lin[e] = pos; elin[pos] = e;
}
// The separator that ends chromosome c carries the CURRENT length of c as its position: the next stage's DNASequence is built from the
// simplified records and stamps it with record[chr].size() (dnasequence.cpp:96), and Replace clamps interpolated positions to the
// position of the element after the rewritten span -- at a chromosome's end that is this separator.
__global__ void k_sep_positions(const unsigned *__restrict__ sepidx, unsigned nchr, unsigned *__restrict__ op)
{
	unsigned i = blockIdx.x * blockDim.x + threadIdx.x;
	if (i < nchr) op[sepidx[i + 1]] = (sepidx[i + 1] - sepidx[i] - 1u) & BT_POS_MASK;
}
// IndexedSequence::Test() (reference src/indexedsequence.cpp:74-103, compiled under _DEBUG only): after any number of collapses, at every
// window position the stored mark equals what the dictionary of the INITIAL marking (k-mer string -> id, FormDictionary) says about the
// k characters spelled there NOW -- "same k-mer => same id everywhere" -- and a position whose k-mer is not in the dictionary (or that
// has no full window) carries no mark.  k <= 32: the dictionary is the sorted list of strand-specific bifurcation codes of the stage's
// enumeration (id = rank).  Checked on the stage's final graph: marks by old slot, characters of the copy-back's linear order.
// out: [0] windows checked, [1] mismatches, [2..5] first mismatch (slot, strand, stored, expected).   SBL_CHECK_DICTIONARY=1.
__device__ __forceinline__ unsigned dict_lookup(const unsigned long long *__restrict__ dict, unsigned nd, unsigned long long code)
{
	unsigned lo = 0, hi = nd;
	while (lo < hi) { unsigned mid = (lo + hi) >> 1; if (dict[mid] < code) lo = mid + 1; else hi = mid; }
	return lo < nd && dict[lo] == code ? lo : BT_NONE;
}
__global__ void __launch_bounds__(256) k_dict_check(const uint8_t *__restrict__ ch, unsigned ne, const unsigned *__restrict__ newidx, const uint8_t *__restrict__ ch_out, unsigned long long total,
                                                    const unsigned *__restrict__ bif0, const unsigned *__restrict__ bif1, const unsigned long long *__restrict__ dict, unsigned nd, unsigned k,
                                                    unsigned long long *__restrict__ out)
{
	const unsigned e = blockIdx.x * blockDim.x + threadIdx.x;
	unsigned checked = 0, bad = 0;
	if (e < ne && ch[e] != BT_DEAD_CHAR && ch[e] != BT_SEP) {
		const unsigned long long p = newidx[e];
		auto base = [](uint8_t c) { unsigned x = (c >> 1) & 3u; return x ^ (x >> 1); };      // A0 C1 G2 T3 (k_pack2bit)
		unsigned exp0 = BT_NONE, exp1 = BT_NONE;
		if (p + k <= total) {
			unsigned long long code = 0; bool full = true;
			for (unsigned i = 0; i < k; i++) { const uint8_t c = ch_out[p + i]; if (c == BT_SEP) { full = false; break; } code = (code << 2) | base(c); }
			if (full) { exp0 = dict_lookup(dict, nd, code); checked++; }
		}
		if (p + 1 >= k) {
			unsigned long long code = 0; bool full = true;
			for (unsigned i = 0; i < k; i++) { const uint8_t c = ch_out[p - i]; if (c == BT_SEP) { full = false; break; } code = (code << 2) | (3u - base(c)); }
			if (full) { exp1 = dict_lookup(dict, nd, code); checked++; }
		}
		const unsigned s0 = bif0[e], s1 = bif1[e];
		if (s0 != exp0) { bad++; if (atomicCAS(&out[2], ~0ull, (unsigned long long)e) == ~0ull) { out[3] = 0; out[4] = s0; out[5] = exp0; } }
		if (s1 != exp1) { bad++; if (atomicCAS(&out[2], ~0ull, (unsigned long long)e) == ~0ull) { out[3] = 1; out[4] = s1; out[5] = exp1; } }
	}
	for (int d = 32; d > 0; d >>= 1) { checked += __shfl_down(checked, d); bad += __shfl_down(bad, d); }
	if ((threadIdx.x & 63) == 0) { if (checked) atomicAdd(&out[0], (unsigned long long)checked); if (bad) atomicAdd(&out[1], (unsigned long long)bad); }
}
__global__ void __launch_bounds__(256) k_fill_bytes(uint8_t *p, uint8_t v, size_t from, size_t to)
{
	size_t i = from + (size_t)blockIdx.x * blockDim.x + threadIdx.x;
	if (i < to) p[i] = v;
}

// ------------------------------------------------------------------------------------------- device backend
// ---- block index over the original slots (GraphView::bidx) -----------------------------------------------------------------------
// Built once per stage from the arrays (and again after a roll-back); from then on the transactions keep it up to date
// (bt_idx_mark / bt_idx_dirty / bt_idx_wstamp).  One wave per block of 64 slots.
__global__ void __launch_bounds__(256) k_build_blkidx(const uint8_t *__restrict__ ch, const unsigned *__restrict__ nx, const unsigned *__restrict__ pv,
                                                      const unsigned *__restrict__ bif0, const unsigned *__restrict__ bif1, unsigned norig, unsigned nblk,
                                                      unsigned long long *__restrict__ bidx)
{
	const unsigned blk = blockIdx.x * 4u + (threadIdx.x >> 6), lane = threadIdx.x & 63u;
	if (blk >= nblk) return;
	const unsigned e = blk * 64u + lane;
	const bool in = e < norig;
	const uint8_t c = in ? ch[e] : (uint8_t)BT_DEAD_CHAR;
	const unsigned long long m0 = __ballot(in && bif0[e] != BT_NONE), m1 = __ballot(in && bif1[e] != BT_NONE), sp = __ballot(in && c == BT_SEP);
	const bool bad = in && (c == BT_DEAD_CHAR || (e + 1u < norig && nx[e] != e + 1u) || (e > 0u && pv[e] != e - 1u));
	const unsigned long long dirty = __ballot(bad) ? 1ull << 32 : 0ull;
	if (lane == 0) {
		unsigned long long *w = bidx + (size_t)blk * BT_IDX_WORDS;
		w[0] = m0; w[1] = m1; w[2] = sp; w[3] = dirty;
	}
}
// SBL_CHECK_INDEX=1 (tests): the maintained index against a rebuild -- marks and separators exactly, "not pristine" and the write
// stamps at least what the arrays show.  out[0] = blocks that differ, out[1] = first of them.
__global__ void __launch_bounds__(256) k_check_blkidx(const uint8_t *__restrict__ ch, const unsigned *__restrict__ nx, const unsigned *__restrict__ pv,
                                                      const unsigned *__restrict__ bif0, const unsigned *__restrict__ bif1, const unsigned *__restrict__ wmax, unsigned norig, unsigned nblk,
                                                      const unsigned long long *__restrict__ bidx, unsigned *__restrict__ out)
{
	const unsigned blk = blockIdx.x * 4u + (threadIdx.x >> 6), lane = threadIdx.x & 63u;
	if (blk >= nblk) return;
	const unsigned e = blk * 64u + lane;
	const bool in = e < norig;
	const uint8_t c = in ? ch[e] : (uint8_t)BT_DEAD_CHAR;
	const unsigned long long m0 = __ballot(in && bif0[e] != BT_NONE), m1 = __ballot(in && bif1[e] != BT_NONE), sp = __ballot(in && c == BT_SEP);
	const bool bad = in && (c == BT_DEAD_CHAR || (e + 1u < norig && nx[e] != e + 1u) || (e > 0u && pv[e] != e - 1u));
	const bool dirty = __ballot(bad) != 0ull;
	unsigned wm = in ? wmax[e] : 0u;
	for (int d = 32; d > 0; d >>= 1) { const unsigned v = __shfl_xor(wm, d); wm = v > wm ? v : wm; }
	if (lane == 0) {
		const unsigned long long *w = bidx + (size_t)blk * BT_IDX_WORDS;
		const bool ok = w[0] == m0 && w[1] == m1 && w[2] == sp && (!dirty || (w[3] >> 32)) && (unsigned)w[3] >= wm;
		if (!ok) { atomicAdd(&out[0], 1u); atomicMin(&out[1], blk); }
	}
}
// everything but the pool cursors (CTR_NE, CTR_NN) back to its start value (DeviceBackend::clear_counters)
__global__ void __launch_bounds__(256) k_clear_counters(unsigned *__restrict__ ctr)
{
	for (unsigned i = CTR_ERR + threadIdx.x; i < CTR_COUNT; i += 256) ctr[i] = i == CTR_VIOL ? BT_NONE : 0u;
}
// What the start of every iteration attempt resets besides rmax / wmax (DeviceBackend::reset_round_state), in ONE launch -- these were
// three fills and two kernels of a few microseconds each: the owners (own = NONE), the parked transactions (park_of, slice_busy = 0;
// nullptr: parking is off), the write stamps of the block index (nullptr: no index) and the counters (k_clear_counters).
__global__ void __launch_bounds__(256) k_reset_iteration(unsigned *__restrict__ ctr, unsigned *__restrict__ own, unsigned *__restrict__ park_of, unsigned nidp,
                                                         uint8_t *__restrict__ slice_busy, unsigned nslices, unsigned long long *__restrict__ bidx, unsigned nblk)
{
	const unsigned i0 = blockIdx.x * blockDim.x + threadIdx.x, stride = gridDim.x * blockDim.x;
	if (blockIdx.x == 0) for (unsigned i = CTR_ERR + threadIdx.x; i < CTR_COUNT; i += 256) ctr[i] = i == CTR_VIOL ? BT_NONE : 0u;
	for (unsigned i = i0; i < nidp; i += stride) { own[i] = BT_NONE; if (park_of) park_of[i] = 0u; }
	if (slice_busy) for (unsigned i = i0; i < nslices; i += stride) slice_busy[i] = 0;
	if (bidx) for (unsigned i = i0; i < nblk; i += stride) reinterpret_cast<unsigned *>(bidx + (size_t)i * BT_IDX_WORDS + 3)[0] = 0u;
}

