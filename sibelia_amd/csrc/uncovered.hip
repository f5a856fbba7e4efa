// uncovered.hip -- what the reference's comparison tool C-Sibelia.py calls from the regions no block covers (src/csibelia/C-Sibelia.py
// :325-338 depict_coverage, :373-427 the walk over the uncovered runs), and the kernel that spells the text of its reports.
//
//   sbl_uncovered_calls   HOST.  C-Sibelia paints one array cell per base; here the same result comes from intervals: per list the ids
//           with an instance on and an instance off the reference records (mixed), the union of their instances per record by one sort,
//           the complement runs longer than min_block_size, and for a run of an assembly record the mixed instance of the FINAL list that
//           holds the base before it (the largest id: C-Sibelia's last writer) with the rule that anchors the insertion.  The host is the
//           right place: the number of runs follows the number of block instances, not of bases, the block lists are host arrays already
//           and nothing here touches a base -- the division DESIGN.md 0.3 argues for the merge of the gap slots.
//   sbl_spell_text        DEVICE.  The calls are written out base by base (REF / ALT of a VCF line, the FASTA of the unmapped insertions:
//           as many bytes as the regions hold), and the host does not keep the records after loading -- so the text is produced where the
//           records are, as blocks_sequences.fasta is (blockseq.hip).  The caller gives an ordered list of PIECES: a range of a blob of
//           literal text, a forward range of an original record copied upper-cased, or such a range wrapped into lines.
//   kernel  k_spell_text, output-stationary like k_block_sequences: a lane owns one 16-byte-aligned 16-byte piece of the text and writes
//           it with ONE vector store; a workgroup owns ST_SPAN contiguous bytes, finds the first and last piece of its span by binary
//           search over the text offsets and keeps their descriptors in LDS (a span of more than ST_LDS pieces -- many literals of a
//           few bytes -- is served from global memory).  A lane wholly inside a record range loads the two aligned 16-byte words its
//           bases come from, shifts them in registers and upper-cases 8 bytes at a time; in a wrapped range `line = off / (width + 1),
//           col = off % (width + 1)` is derived once per lane.  Lanes on piece boundaries, in literals and in ranges wrapped narrower
//           than 16 step byte by byte.
//   back    through the context's pinned staging buffer for device-made text (sbl_text_staging, blockseq.hip).
#include <algorithm>
#include <cstring>

#include "sbl_align.h"
#include "sbl_text.h"

namespace {

constexpr unsigned ST_THREADS = 256, ST_SPAN = ST_THREADS * 16, ST_LDS = 128;

struct StDesc {
	u64 src;                         // record range: element index of its first base in d_orig_ch; literal: offset in the blob
	u64 L;                           // bases / literal bytes
	unsigned width, literal;         // width > 0: a '\n' after every `width` bases and one after the last
};

// str.upper() on 8 ASCII bytes at once: 'a' .. 'z' lose 0x20, every other byte (those above 0x7F too) is unchanged
__device__ inline u64 upper8(u64 x)
{
	const u64 low7 = x & 0x7F7F7F7F7F7F7F7Full;
	const u64 ge_a = low7 + 0x1F1F1F1F1F1F1F1Full;                        // 0x80 set where low7 >= 'a' (0x61); no carry leaves a byte
	const u64 gt_z = low7 + 0x0505050505050505ull;                        // ... where low7 > 'z' (0x7A)
	return x ^ ((ge_a & ~gt_z & ~x & 0x8080808080808080ull) >> 2);
}
__device__ inline unsigned char upper1(unsigned char c) { return c >= 'a' && c <= 'z' ? c ^ 0x20 : c; }

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
	bool fast = !d.literal && off + 16 <= tlen && (d.width == 0 || d.width >= 16);
	u64 base = off;
	unsigned nl = 16;                                                     // where a line feed falls in the piece (16: nowhere)
	if (fast && d.width) {
		// a line is width + 1 >= 17 bytes (64-bit: width is the caller's): at most one line feed of a full line in the piece, and perhaps the one after the last base
		const u64 line = off / ((u64)d.width + 1);
		const unsigned col = (unsigned)(off % ((u64)d.width + 1));
		const unsigned full = d.width - col;                                // col == width: the piece starts on the line feed
		const u64 last = tlen - 1 - off;                                    // >= 15
		base = line * d.width + col;
		if (full < 16 && last < 16 && full != last) fast = false;          // both: a last line of a few bases
		else nl = full < 16 ? full : last < 16 ? (unsigned)last : 16;
	}
	if (fast) {
		// ---- the whole piece is bases (and at most one line feed) of one record range
		const u64 s0 = d.src + base;
		const uint4 *p = reinterpret_cast<const uint4 *>(orig + (s0 & ~15ull));
		w = window16(p[0], p[1], (unsigned)(s0 & 15));
		w.lo = upper8(w.lo); w.hi = upper8(w.hi);
		if (nl < 16) w = insert_newline(w, nl);
	} else {
		// ---- literals, boundaries between pieces, short pieces, narrow lines: byte by byte, (base, col) stepped
		w.lo = w.hi = 0;
		unsigned col = 0; bool entered = false;
		for (unsigned j = 0; j < 16 && t0 + j < total; j++) {
			while (off == tlen) { di++; d = D[di]; off = 0; tlen = O[di + 1] - O[di]; entered = false; }
			unsigned char ch;
			if (d.literal) ch = (unsigned char)literals[d.src + off];
			else if (!d.width) ch = upper1(orig[d.src + off]);
			else {
				if (!entered) { col = (unsigned)(off % ((u64)d.width + 1)); base = off / ((u64)d.width + 1) * d.width + col; entered = true; }
				if (off + 1 == tlen || col == d.width) { ch = '\n'; col = 0; }
				else { ch = upper1(orig[d.src + base]); base++; col++; }
			}
			if (j < 8) w.lo |= (u64)ch << (8 * j); else w.hi |= (u64)ch << (8 * (j - 8));
			off++;
		}
	}
	out[t0 / 16] = make_uint4((unsigned)w.lo, (unsigned)(w.lo >> 32), (unsigned)w.hi, (unsigned)(w.hi >> 32));
}

struct Iv { uint32_t chr; int32_t id; uint64_t start, end; };             // one instance of a mixed block; id = |block id|

// the instances of the mixed blocks of one list: blocks with an instance on and an instance off the reference records
void mixed_instances(const sbl_block *b, uint64_t n, uint32_t nref, std::vector<Iv> &out)
{
	std::vector<sbl_block> v(b, b + n);
	std::stable_sort(v.begin(), v.end(), [](const sbl_block &x, const sbl_block &y) { return std::abs(x.id) < std::abs(y.id); });
	for_each_id_run(v, [&](size_t i, size_t j) {
		size_t on = 0;
		for (size_t k = i; k < j; k++) on += v[k].chr < nref;
		if (on == 0 || on == j - i) return;
		for (size_t k = i; k < j; k++)
			if (v[k].end > v[k].start) out.push_back(Iv{v[k].chr, std::abs(v[k].id), v[k].start, v[k].end});      // an empty instance holds no base
	});
}

bool by_start(const Iv &x, const Iv &y) { return x.chr != y.chr ? x.chr < y.chr : x.start < y.start; }

}  // namespace

extern "C" sbl_status sbl_uncovered_calls(sbl_ctx *c, uint64_t nlists, const uint64_t *list_first, const sbl_block *blocks, uint32_t min_block_size,
                                          uint32_t n_reference_chr, const sbl_uncovered_call **calls, uint64_t *ncalls)
{
	return guarded(c, [&] {
		require_records(c);
		require_reference_split(c, n_reference_chr);
		SBL_CHECK(nlists >= 1 && list_first, SBL_ERR_BAD_ARG, "at least one block list (the final one) is needed");
		SBL_CHECK(list_first[0] == 0, SBL_ERR_BAD_ARG, "the first list starts at 0");
		for (uint64_t l = 0; l < nlists; l++) SBL_CHECK(list_first[l] <= list_first[l + 1], SBL_ERR_BAD_ARG, "list offsets must ascend");
		sbl_check_blocks(c, blocks, list_first[nlists]);
		const uint32_t nref = n_reference_chr;
		const uint64_t m = min_block_size;

		// coverage: the mixed instances of EVERY list; main: those of the last one
		std::vector<Iv> cover, fin;
		for (uint64_t l = 0; l < nlists; l++) mixed_instances(blocks + list_first[l], list_first[l + 1] - list_first[l], nref, l + 1 == nlists ? fin : cover);
		cover.insert(cover.end(), fin.begin(), fin.end());
		std::sort(cover.begin(), cover.end(), by_start);
		std::sort(fin.begin(), fin.end(), by_start);
		// reach[i]: the farthest end among fin[first of the record .. i] -- where a walk downwards from i may stop
		std::vector<uint64_t> reach(fin.size());
		std::vector<size_t> fin_first(c->nchr + 1);                       // fin[fin_first[r], fin_first[r + 1]): record r
		for (size_t r = 0, k = 0; r <= c->nchr; r++) {
			while (k < fin.size() && fin[k].chr < r) k++;
			fin_first[r] = k;
		}
		for (size_t i = 0; i < fin.size(); i++) reach[i] = i && fin[i - 1].chr == fin[i].chr ? std::max(reach[i - 1], fin[i].end) : fin[i].end;
		// the final list by |id|, for the anchor rule
		const sbl_block *fb = blocks + list_first[nlists - 1];
		std::vector<sbl_block> byid(fb, fb + (list_first[nlists] - list_first[nlists - 1]));
		std::stable_sort(byid.begin(), byid.end(), [](const sbl_block &x, const sbl_block &y) { return std::abs(x.id) < std::abs(y.id); });

		// main(x) on record r: the largest id among the final mixed instances that hold base x, 0 if there is none
		auto main_at = [&](uint32_t r, uint64_t x) {
			const Iv key{r, 0, x, 0};
			size_t i = std::upper_bound(fin.begin() + fin_first[r], fin.begin() + fin_first[r + 1], key, by_start) - fin.begin();
			int32_t best = 0;
			while (i-- > fin_first[r] && reach[i] > x)
				if (fin[i].end > x) best = std::max(best, fin[i].id);
			return best;
		};
		std::vector<sbl_uncovered_call> &out = c->unc_calls;
		out.clear();
		auto run = [&](uint32_t r, uint64_t s, uint64_t e) {
			if (e - s <= m) return;
			sbl_uncovered_call u{};
			u.chr = r; u.start = s; u.end = e;
			if (r < nref) { u.kind = SBL_CALL_DELETION; u.ref_chr = r; u.pos = s; out.push_back(u); return; }
			u.kind = SBL_CALL_UNMAPPED;
			const int32_t b = s ? main_at(r, s - 1) : 0;
			if (b) {
				const auto range = std::equal_range(byid.begin(), byid.end(), sbl_block{b, 0, 0, 0},
				                                    [](const sbl_block &x, const sbl_block &y) { return std::abs(x.id) < std::abs(y.id); });
				const sbl_block *i = &*range.first;
				// determine_unique_block (C-Sibelia.py:314-323), as sbl_align_unique_blocks applies it
				if (range.second - range.first == 2 && (i[0].chr < nref) != (i[1].chr < nref)) {
					const sbl_block &a = i[0].chr < nref ? i[0] : i[1], &o = i[0].chr < nref ? i[1] : i[0];
					if (a.end - a.start >= m && o.end - o.start >= m) {
						const uint64_t p = (a.id < 0) == (o.id < 0) ? a.end : a.start;
						if (p > 0) { u.kind = SBL_CALL_INSERTION; u.ref_chr = a.chr; u.pos = p; }
					}
				}
			}
			out.push_back(u);
		};
		size_t i = 0;
		for (uint32_t r = 0; r < c->nchr; r++) {
			const uint64_t size = (uint64_t)(c->orig_sepidx[r + 1] - c->orig_sepidx[r] - 1);
			uint64_t at = 0;                                                 // everything before `at` is covered or reported
			for (; i < cover.size() && cover[i].chr == r; i++) {
				if (cover[i].start > at) run(r, at, cover[i].start);
				at = std::max(at, cover[i].end);
			}
			if (size > at) run(r, at, size);
		}
		if (calls) *calls = out.data();
		if (ncalls) *ncalls = out.size();
	});
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
			u64 len;
			if (p.kind == SBL_PIECE_LITERAL) {
				SBL_CHECK(p.start <= p.end && p.end <= literal_len, SBL_ERR_BAD_ARG, "a literal piece outside the literal text");
				SBL_CHECK(p.width == 0, SBL_ERR_BAD_ARG, "a literal piece is not wrapped");
				d.src = p.start; d.L = len = p.end - p.start; d.literal = 1;
			} else {
				SBL_CHECK(p.kind == SBL_PIECE_RECORD, SBL_ERR_BAD_ARG, "unknown kind of piece");
				check_range(c, p.chr, p.start, p.end, "a piece on a record that does not exist");
				d.src = (u64)c->orig_sepidx[p.chr] + 1 + p.start; d.L = p.end - p.start; d.width = p.width;
				len = d.L + (p.width ? (d.L + p.width - 1) / p.width : 0);
			}
			if (!len) continue;
			desc.push_back(d);
			toff.push_back(toff.back() + len);
		}
		const u64 total = toff.back(), n = desc.size();
		if (total) {
			hipStream_t s = c->stream;
			const size_t padded = (size_t)((total + 15) / 16 * 16);
			const uint64_t groups = (total + ST_SPAN - 1) / ST_SPAN;
			SBL_CHECK(groups < 0x7FFFFFFFull, SBL_ERR_TOO_LARGE, "text too large");
			c->d_bs_desc.ensure(n * sizeof(StDesc)); c->d_bs_off.ensure((n + 1) * 8); c->d_bs_hdr.ensure(std::max<size_t>(1, literal_len)); c->d_bs_text.ensure(padded);
			sbl_text_staging(c, padded);
			HIP_TRY(hipMemcpyAsync(c->d_bs_desc.p, desc.data(), n * sizeof(StDesc), hipMemcpyHostToDevice, s));
			HIP_TRY(hipMemcpyAsync(c->d_bs_off.p, toff.data(), (n + 1) * 8, hipMemcpyHostToDevice, s));
			if (literal_len) HIP_TRY(hipMemcpyAsync(c->d_bs_hdr.p, literals, literal_len, hipMemcpyHostToDevice, s));
			HIP_TRY(hipEventRecord(c->ev[0], s));
			k_spell_text<<<(unsigned)groups, ST_THREADS, 0, s>>>(c->d_orig_ch.as<uint8_t>(), c->d_bs_desc.as<StDesc>(), c->d_bs_off.as<u64>(), n,
			                                                   c->d_bs_hdr.as<char>(), total, c->d_bs_text.as<uint4>());
			HIP_TRY(hipGetLastError());
			HIP_TRY(hipEventRecord(c->ev[1], s));
			HIP_TRY(hipMemcpyAsync(c->h_bs_text, c->d_bs_text.p, padded, hipMemcpyDeviceToHost, s));
			HIP_TRY(hipEventRecord(c->ev[2], s));
			HIP_TRY(hipStreamSynchronize(s));
			float k_ms = 0, d_ms = 0;
			(void)hipEventElapsedTime(&k_ms, c->ev[0], c->ev[1]);
			(void)hipEventElapsedTime(&d_ms, c->ev[1], c->ev[2]);
			c->st_kernel_ms = k_ms; c->st_copy_ms = d_ms;
			c->stats.device_bytes = sbl_devbuf_total().load();
		}
		if (text) *text = total ? c->h_bs_text : "";
		if (text_len) *text_len = total;
	});
}

extern "C" sbl_status sbl_spell_text_times(const sbl_ctx *c, double *kernel_ms, double *copyback_ms)
{
	if (!c) return SBL_ERR_BAD_ARG;
	if (kernel_ms) *kernel_ms = c->st_kernel_ms;
	if (copyback_ms) *copyback_ms = c->st_copy_ms;
	return SBL_OK;
}
