// sbl_text.h -- the text kernel's tools (spell_text.hip: k_spell_text): the search of a text offset in the offsets of the pieces, and
// 16 bytes of text held in two registers -- cut out of two aligned source words (gv_load16: the readers of the alignment rows,
// sbl_groups.h), complemented, opened for a line feed, stored as one vector (store16).  And the pieces k_spell_text spells, with the one
// host function that launches it for sbl_spell_text (spell_text.hip) and sbl_blocks_sequences (blockseq.hip).
#pragma once
#include <hip/hip_runtime.h>

#include <vector>

typedef unsigned long long u64;

// one piece of text, never empty.  Properties of the piece, whoever asks for it:
constexpr unsigned ST_LITERAL = 1;   // a range of the blob, copied as it is (width 0); otherwise a range of the original records
constexpr unsigned ST_REVERSE = 2;   // the range is read downwards through the complement (DNASequence::Translate)
constexpr unsigned ST_KEEP_CASE = 4; // the bases keep their case; otherwise they are upper-cased
struct StDesc {
	u64 src;                         // record range: element index of its first base in d_orig_ch; literal: offset in the blob
	u64 L;                           // bases / literal bytes
	unsigned width, flags;           // width > 0: a '\n' after every `width` bases and one after the last
};
inline u64 st_text_len(u64 L, unsigned width) { return L + (width ? (L + width - 1) / width : 0); }

struct sbl_ctx;
struct SblTimes;
// The text of the pieces `desc` (toff: their desc.size() + 1 text offsets, toff[0] = 0; blob: what the literal pieces cut from) into
// h_bs_text, the context's staging buffer: uploads, k_spell_text and the copy back between event pairs, one synchronise.  `t`: the
// times of the kernel and of the copy, untouched when there is no text.  too_large: the caller's words for a text beyond the grid.
void sbl_spell_pieces(sbl_ctx *c, const std::vector<StDesc> &desc, const std::vector<u64> &toff, const char *blob, size_t blob_len, const char *too_large, SblTimes &t);

// largest i in [0, n) with off[i] <= x (off[0] = 0 <= x)
template <class P> __device__ inline unsigned bs_find(P off, unsigned long long n, u64 x)
{
	unsigned long long lo = 0, hi = n;
	while (hi - lo > 1) {
		const unsigned long long mid = lo + (hi - lo) / 2;
		if (off[mid] <= x) lo = mid; else hi = mid;
	}
	return (unsigned)lo;
}

// zero8: 0x80 in every byte of v that is zero (exact: no carries cross bytes)
__device__ inline u64 zero8(u64 v) { return ~(((v & 0x7F7F7F7F7F7F7F7Full) + 0x7F7F7F7F7F7F7F7Full) | v) & 0x8080808080808080ull; }
// 0x80 in every byte of v that is not zero
__device__ inline u64 nonzero8(u64 v) { return ~zero8(v) & 0x8080808080808080ull; }
// 0x80 in every byte of v that is one of A C G T, 0x40 in every byte that is '-' (group_distances.hip, group_concat.hip)
__device__ inline u64 base_flags8(u64 v)
{
	const u64 base = zero8(v ^ 0x4141414141414141ull) | zero8(v ^ 0x4343434343434343ull) | zero8(v ^ 0x4747474747474747ull) | zero8(v ^ 0x5454545454545454ull);
	return base | (zero8(v ^ 0x2D2D2D2D2D2D2D2Dull) >> 1);
}

// DNASequence::Translate (src/dnasequence.cpp:11-28) on 8 bytes at once: A <-> T and C <-> G in either case, every other byte unchanged.
__device__ inline u64 complement8(u64 x)
{
	const u64 f = x & 0xDFDFDFDFDFDFDFDFull;                            // case folded: 0x41 only for 'A' / 'a', ...
	const u64 at = (zero8(f ^ 0x4141414141414141ull) | zero8(f ^ 0x5454545454545454ull)) >> 7;
	const u64 cg = (zero8(f ^ 0x4343434343434343ull) | zero8(f ^ 0x4747474747474747ull)) >> 7;
	return x ^ (at * 0x15) ^ (cg * 0x04);                               // 'A' ^ 'T' = 0x15, 'C' ^ 'G' = 0x04
}

struct B16 { u64 lo, hi; };
// the one vector store of an output-stationary lane: w as the 16-byte word `word` of out
__device__ inline void store16(uint4 *__restrict__ out, u64 word, B16 w) { out[word] = make_uint4((unsigned)w.lo, (unsigned)(w.lo >> 32), (unsigned)w.hi, (unsigned)(w.hi >> 32)); }
// bytes [sh, sh + 16) of the 32 bytes (a, b), sh in [0, 16)
__device__ inline B16 window16(uint4 a, uint4 b, unsigned sh)
{
	u64 w0 = (u64)a.x | ((u64)a.y << 32), w1 = (u64)a.z | ((u64)a.w << 32), w2 = (u64)b.x | ((u64)b.y << 32), w3 = (u64)b.z | ((u64)b.w << 32);
	if (sh >= 8) { w0 = w1; w1 = w2; w2 = w3; sh -= 8; }
	if (!sh) return {w0, w1};
	const unsigned r = sh * 8;
	return {(w0 >> r) | (w1 << (64 - r)), (w1 >> r) | (w2 << (64 - r))};
}
// bytes [at, at + 16) of text as two 64-bit words; words that lie wholly beyond text[0, bytes) are not loaded (bytes: a multiple of 16)
__device__ inline B16 gv_load16(const uint8_t *__restrict__ text, u64 bytes, u64 at)
{
	const u64 base = at & ~15ull;
	const unsigned sh = (unsigned)(at & 15);
	const uint4 zero = make_uint4(0, 0, 0, 0);
	const uint4 a = base < bytes ? *reinterpret_cast<const uint4 *>(text + base) : zero;
	const uint4 b = sh && base + 16 < bytes ? *reinterpret_cast<const uint4 *>(text + base + 16) : zero;
	return window16(a, b, sh);
}
// 16 bytes with '\n' inserted before byte p (p in [0, 16)); the last byte falls off
__device__ inline B16 insert_newline(B16 w, unsigned p)
{
	B16 o;
	if (p < 8) {
		const unsigned r = p * 8;
		const u64 keep = r ? w.lo & (~0ull >> (64 - r)) : 0;
		const u64 up = r ? (w.lo >> r) << r : w.lo;                       // bytes p.. of lo
		o.lo = keep | ((u64)'\n' << r) | (up << 8);
		o.hi = (w.hi << 8) | (w.lo >> 56);
	} else {
		const unsigned r = (p - 8) * 8;
		const u64 keep = r ? w.hi & (~0ull >> (64 - r)) : 0;
		const u64 up = r ? (w.hi >> r) << r : w.hi;
		o.lo = w.lo;
		o.hi = keep | ((u64)'\n' << r) | (up << 8);
	}
	return o;
}
