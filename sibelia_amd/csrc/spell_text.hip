// spell_text.hip -- text put together on the device from the ORIGINAL records (d_orig_ch, kept since sbl_load / sbl_load_fasta): the one
// kernel behind blocks_sequences.fasta (sbl_blocks_sequences, blockseq.hip) and behind the reports of --uncovered (sbl_spell_text, here).
//
// These are the reports whose size scales with the input -- every block instance, every uncovered region is written out base by base --
// and the host never holds the parsed records after sbl_load_fasta, so the text is produced where the sequences are.  A caller gives an
// ordered list of PIECES (StDesc, sbl_text.h): a range of a blob of literal text, or a range of an original record -- forwards or
// downwards through the complement, upper-cased or as it is, in one run or wrapped into lines.
//
//   kernel  k_spell_text, output-stationary: a lane owns one 16-byte-aligned 16-byte piece of the text and writes it with ONE vector
//           store; a workgroup owns ST_SPAN contiguous bytes, finds the first and last piece of its span by binary search over the text
//           offsets and keeps their descriptors in LDS (a span of more than ST_LDS pieces -- many literals of a few bytes -- is served
//           from global memory).  A lane wholly inside a record range loads the two aligned 16-byte words its bases come from --
//           neighbouring lanes read neighbouring words, ascending for a forward and descending for a reverse range, so the wave's reads
//           stay coalesced either way -- and shifts, reverses, complements and upper-cases them in registers, 8 bytes at a time; in a
//           wrapped range `line = off / (width + 1), col = off % (width + 1)` is derived once per lane.  Lanes on piece boundaries, in
//           literals and in ranges wrapped narrower than 16 step byte by byte.
//   host    sbl_spell_pieces: descriptors, offsets and blob go up once; the kernel and the copy back lie between event pairs
//   back    through a pinned staging buffer owned by the context (sbl_text_staging: HostText, pageable when pinning fails).
#include <algorithm>

#include "sbl_align.h"
#include "sbl_text.h"

namespace {

constexpr unsigned ST_THREADS = 256, ST_SPAN = ST_THREADS * 16, ST_LDS = 256;

// str.upper() on 8 ASCII bytes at once: 'a' .. 'z' lose 0x20, every other byte (those above 0x7F too) is unchanged
__device__ inline u64 upper8(u64 x)
{
	const u64 low7 = x & 0x7F7F7F7F7F7F7F7Full;
	const u64 ge_a = low7 + 0x1F1F1F1F1F1F1F1Full;                        // 0x80 set where low7 >= 'a' (0x61); no carry leaves a byte
	const u64 gt_z = low7 + 0x0505050505050505ull;                        // ... where low7 > 'z' (0x7A)
	return x ^ ((ge_a & ~gt_z & ~x & 0x8080808080808080ull) >> 2);
}
__device__ inline unsigned char upper1(unsigned char c) { return c >= 'a' && c <= 'z' ? c ^ 0x20 : c; }

// base i of a record range as the piece spells it
__device__ inline unsigned char piece_base(const uint8_t *__restrict__ orig, const StDesc &d, u64 i)
{
	const unsigned char ch = d.flags & ST_REVERSE ? complement1(orig[d.src + d.L - 1 - i]) : orig[d.src + i];
	return d.flags & ST_KEEP_CASE ? ch : upper1(ch);
}

__global__ __launch_bounds__(ST_THREADS) void k_spell_text(const uint8_t *__restrict__ orig, const StDesc *__restrict__ desc,
                                                           const u64 *__restrict__ toff /* n + 1 */, unsigned long long n,
                                                           const char *__restrict__ literals, u64 total, uint4 *__restrict__ out)
{
	__shared__ StDesc s_desc[ST_LDS];
	__shared__ u64 s_off[ST_LDS + 1];
	__shared__ unsigned s_first, s_count;
	const u64 span0 = (u64)blockIdx.x * ST_SPAN;
	if (span0 >= total) return;
	const u64 span1 = span0 + ST_SPAN < total ? span0 + ST_SPAN : total;      // one past the last byte of text in the span
	if (threadIdx.x == 0) s_first = bs_find(toff, n, span0);
	if (threadIdx.x == 1) s_count = bs_find(toff, n, span1 - 1);
	__syncthreads();
	const unsigned first = s_first, count = s_count - first + 1;
	__syncthreads();
	// blocks_sequences.fasta: two pieces (header, bases) per instance, whose text is 46 bytes at least (the reference's header has 44),
	// so a span holds under 184 of them and stays on chip; a list of pieces that defeats ST_LDS is served from global memory instead
	const bool in_lds = count <= ST_LDS;
	if (in_lds) {
		for (unsigned i = threadIdx.x; i < count; i += ST_THREADS) s_desc[i] = desc[first + i];
		for (unsigned i = threadIdx.x; i <= count; i += ST_THREADS) s_off[i] = toff[first + i];
		__syncthreads();
	}
	const StDesc *D = in_lds ? s_desc : desc + first;
	const u64 *O = in_lds ? s_off : toff + first;

	const u64 t0 = span0 + (u64)threadIdx.x * 16;
	if (t0 >= span1) return;
	unsigned di = bs_find(O, count, t0);
	StDesc d = D[di];
	u64 off = t0 - O[di];                                                 // offset inside the piece's text
	u64 tlen = O[di + 1] - O[di];                                         // never 0: the host drops empty pieces
	B16 w;
	bool fast = !(d.flags & ST_LITERAL) && off + 16 <= tlen && (d.width == 0 || d.width >= 16);
	u64 base = off;                                                       // the base of a record range that the text goes on with ...
	unsigned col = 0;                                                     // ... and its place in its line: the one division of the lane (64-bit: width is the caller's)
	if (!(d.flags & ST_LITERAL) && d.width) { col = (unsigned)(off % ((u64)d.width + 1)); base = off / ((u64)d.width + 1) * d.width + col; }
	unsigned nl = 16;                                                     // where a line feed falls in the piece (16: nowhere)
	if (fast && d.width) {
		// a line is width + 1 >= 17 bytes: at most one line feed of a full line in the piece, and perhaps the one after the last base
		const unsigned full = d.width - col;                                // col == width: the piece starts on the line feed
		const u64 last = tlen - 1 - off;                                    // >= 15
		if (full < 16 && last < 16 && full != last) fast = false;          // both: a last line of a few bases
		else nl = full < 16 ? full : last < 16 ? (unsigned)last : 16;
	}
	if (fast) {
		// ---- the whole piece is bases (and at most one line feed) of one record range
		// forward: the 16 bytes from the piece's first base.  Reverse: bases s0, s0 - 1, ..., s0 - 15 with s0 = src + L - 1 - base -- the 16
		// bytes ending at s0, reversed and complemented.  They start at a0 >= d.src - 1 >= 0: the piece holds at least 15 bases (16 bytes of
		// text, one line feed at most -- that of a full line or the one after the last base), and element 0 of the records is the '$'
		// before the first
		const bool rev = d.flags & ST_REVERSE;
		const u64 a0 = rev ? d.src + d.L - 16 - base : d.src + base;
		const uint4 *p = reinterpret_cast<const uint4 *>(orig + (a0 & ~15ull));
		w = window16(p[0], p[1], (unsigned)(a0 & 15));
		if (rev) w = B16{complement8(__builtin_bswap64(w.hi)), complement8(__builtin_bswap64(w.lo))};
		if (!(d.flags & ST_KEEP_CASE)) { w.lo = upper8(w.lo); w.hi = upper8(w.hi); }
		if (nl < 16) w = insert_newline(w, nl);
	} else {
		// ---- literals, boundaries between pieces, short pieces, narrow lines: byte by byte, (base, col) stepped
		w.lo = w.hi = 0;
		for (unsigned j = 0; j < 16 && t0 + j < total; j++) {
			if (off == tlen) { di++; d = D[di]; off = 0; tlen = O[di + 1] - O[di]; base = 0; col = 0; }      // the next piece, from its start
			unsigned char ch;
			if (d.flags & ST_LITERAL) ch = (unsigned char)literals[d.src + off];
			else if (d.width && (off + 1 == tlen || col == d.width)) { ch = '\n'; col = 0; }
			else { ch = piece_base(orig, d, base); base++; col++; }
			if (j < 8) w.lo |= (u64)ch << (8 * j); else w.hi |= (u64)ch << (8 * (j - 8));
			off++;
		}
	}
	store16(out, t0 / 16, w);
}

}  // namespace

void sbl_spell_pieces(sbl_ctx *c, const std::vector<StDesc> &desc, const std::vector<u64> &toff, const char *blob, size_t blob_len, const char *too_large, SblTimes &t)
{
	const u64 total = toff.back(), n = desc.size();
	if (total) {
		hipStream_t s = c->stream;
		const size_t padded = (size_t)((total + 15) / 16 * 16);
		const uint64_t groups = (total + ST_SPAN - 1) / ST_SPAN;
		SBL_CHECK(groups < 0x7FFFFFFFull, SBL_ERR_TOO_LARGE, too_large);
		c->d_bs_desc.ensure(n * sizeof(StDesc)); c->d_bs_off.ensure((n + 1) * 8); c->d_bs_hdr.ensure(std::max<size_t>(1, blob_len)); c->d_bs_text.ensure(padded);
		sbl_text_staging(c, padded);
		HIP_TRY(hipMemcpyAsync(c->d_bs_desc.p, desc.data(), n * sizeof(StDesc), hipMemcpyHostToDevice, s));
		HIP_TRY(hipMemcpyAsync(c->d_bs_off.p, toff.data(), (n + 1) * 8, hipMemcpyHostToDevice, s));
		if (blob_len) HIP_TRY(hipMemcpyAsync(c->d_bs_hdr.p, blob, blob_len, hipMemcpyHostToDevice, s));
		HIP_TRY(hipEventRecord(c->ev[0], s));
		k_spell_text<<<(unsigned)groups, ST_THREADS, 0, s>>>(c->d_orig_ch.as<uint8_t>(), c->d_bs_desc.as<StDesc>(), c->d_bs_off.as<u64>(), n,
		                                                   c->d_bs_hdr.as<char>(), total, c->d_bs_text.as<uint4>());
		HIP_TRY(hipGetLastError());
		HIP_TRY(hipEventRecord(c->ev[1], s));
		HIP_TRY(hipMemcpyAsync(c->h_bs_text.p, c->d_bs_text.p, padded, hipMemcpyDeviceToHost, s));
		HIP_TRY(hipEventRecord(c->ev[2], s));
		HIP_TRY(hipStreamSynchronize(s));
		t.kernel_ms = sbl_elapsed_ms(c, 0, 1); t.copy_ms = sbl_elapsed_ms(c, 1, 2);
	}
	c->stats.device_bytes = sbl_devbuf_total().load();
}

extern "C" sbl_status sbl_spell_text(sbl_ctx *c, uint64_t npieces, const sbl_text_piece *pieces, const char *literals, uint64_t literal_len,
                                     const char **text, uint64_t *text_len)
{
	return guarded(c, [&] {
		require_records(c);
		SBL_CHECK(npieces == 0 || pieces, SBL_ERR_BAD_ARG, "null piece list");
		SBL_CHECK(literal_len == 0 || literals, SBL_ERR_BAD_ARG, "null literal text");
		// every argument is checked before anything is launched; empty pieces are dropped here (the kernel's pieces all hold text)
		std::vector<StDesc> desc;
		std::vector<u64> toff(1, 0);
		desc.reserve(npieces); toff.reserve(npieces + 1);
		for (uint64_t i = 0; i < npieces; i++) {
			const sbl_text_piece &p = pieces[i];
			StDesc d{};
			if (p.kind == SBL_PIECE_LITERAL) {
				SBL_CHECK(p.start <= p.end && p.end <= literal_len, SBL_ERR_BAD_ARG, "a literal piece outside the literal text");
				SBL_CHECK(p.width == 0, SBL_ERR_BAD_ARG, "a literal piece is not wrapped");
				d.src = p.start; d.L = p.end - p.start; d.flags = ST_LITERAL;
			} else {
				SBL_CHECK(p.kind == SBL_PIECE_RECORD, SBL_ERR_BAD_ARG, "unknown kind of piece");
				check_range(c, p.chr, p.start, p.end, "a piece on a record that does not exist");
				d.src = (u64)c->orig_sepidx[p.chr] + 1 + p.start; d.L = p.end - p.start; d.width = p.width;
			}
			if (!d.L) continue;
			desc.push_back(d);
			toff.push_back(toff.back() + st_text_len(d.L, d.width));
		}
		sbl_spell_pieces(c, desc, toff, literals, literal_len, "text too large", c->st_times);
		if (text) *text = toff.back() ? c->h_bs_text.p : "";
		if (text_len) *text_len = toff.back();
	});
}

extern "C" sbl_status sbl_spell_text_times(const sbl_ctx *c, double *kernel_ms, double *copyback_ms)
{
	return sbl_times_out(c, &sbl_ctx::st_times, kernel_ms, copyback_ms);
}
