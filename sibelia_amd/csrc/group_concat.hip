// group_concat.hip -- the concatenated alignment of the multiple alignments (include/sibelia_amd.h): the rows of the used
// groups of the last sbl_align_groups / sbl_align_block_groups call, group after group, as one FASTA record per CLASS the caller gives
// the instances (the pipeline: the input file) -- all columns (SBL_CONCAT_ALL) or the columns in which all rows hold one of A C G T and
// not all the same (SBL_CONCAT_VARIABLE).  The text is classes x columns bytes, the order of the rows themselves, and the rows lie on
// the device (d_ga_text): a column filter and a transposing gather, so they run where the rows are and only the text comes back.
//
//   flags     (VARIABLE) k_site_flags of sbl_groups.h, its column walk (gm_walk16: a lane owns 16 columns of ONE group, every group padded
//             to a multiple of 16 columns) with "every row holds one of A C G T" (base_flags8) gathered next to "differs from row 0": 16
//             flag bytes per lane.  Padding columns get flag 0.
//   sites     (VARIABLE) the flagged columns are compacted in ascending order by rocPRIM's select (sbl_prim.h); the host reads their
//             number; k_site_fill, one lane per site: the group by binary search over the padded prefix, `before` from the group's merged
//             gap slots (gm_centre_before), and for the text kernel the pick (used group, column).
//   text      k_concat_text, output-stationary like k_spell_text: a lane owns 16 aligned bytes of the text and makes ONE vector store; a
//             workgroup owns GC_SPAN contiguous bytes and keeps the text offsets of the class rows its span touches in LDS (they differ
//             only by the header lengths).  A lane finds its class by search over them, then header (literal bytes) or sequence, where
//             `line = off / (width + 1), col = off % (width + 1)` is derived once.  ALL: the group by bs_find over the parts' first
//             columns, the source row through roff[used group][class], the start of that class's row of the group in d_ga_text, built on
//             the host from cls; 16 bytes inside one group's row are cut out of two aligned words (gv_load16) and opened for a line feed
//             (insert_newline); lanes that straddle a header, a group boundary or two line ends step byte by byte.  VARIABLE: every byte
//             is one scattered load through the picks -- kept columns are a percent or so of all, so the loads are sparse by nature and
//             nothing is staged; the stores stay coalesced.
//   host      every argument is checked before any launch; the used groups by the walk of sbl_groups.h (gm_columns: a group of ONE row is
//             used when there is one class), tables up; event pairs around the kernels and around the copy back; the text comes back
//             into a pinned buffer of its own that grows on demand (h_gc_text), sites into gc_sites; the parts of mode VARIABLE are
//             counted on the host from the sites.
//   partial   under sbl_group_set_partial a used group holds every class at most once: k_site_flags<.., true> walks the
//             rows the group has, and k_concat_text<.., true> writes '-' for a class the group does not hold (roff == ~0).
#include <algorithm>
#include <cstdio>
#include <cstring>

#include "sbl_groups.h"
#include "sbl_prim.h"

namespace {

constexpr unsigned GC_THREADS = GM_THREADS, GC_SPAN = GC_THREADS * 16;

struct GcPick { u64 ug, col; };                        // a kept column: its used group and its column there

__global__ __launch_bounds__(GC_THREADS) void k_site_fill(const GmGroup *__restrict__ gm, const GmSlot *__restrict__ slots, const GmUsed *__restrict__ groups,
                                                          const u64 *__restrict__ cbase, u64 ngroups, const u64 *__restrict__ xs, u64 nsites,
                                                          sbl_concat_site *__restrict__ sites, GcPick *__restrict__ picks)
{
	const u64 i = (u64)blockIdx.x * GC_THREADS + threadIdx.x;
	if (i >= nsites) return;
	const u64 x = xs[i];
	const unsigned gi = bs_find(cbase, ngroups, x);
	const GmGroup Q = gm[groups[gi].dg];
	const u64 s = x - cbase[gi];
	sites[i] = sbl_concat_site{groups[gi].group, s, gm_centre_before(slots, Q, s)};
	picks[i] = GcPick{gi, s};
}

// coff: the nclass + 1 text offsets of the class rows; row f is its header -- hdr[coff[f] - f S ...), S = st_text_len(C, width) -- and the
// S bytes of its C kept columns in lines.  roff[ug * nclass + f]: where the row of class f of used group ug starts in `text`.
// ALL: first[ug] (nused + 1): the first column of the used group in the concatenation.  VARIABLE: picks[C].
// PARTIAL (sbl_group_set_partial): roff == ~0 says that the used group does not hold the class; its bytes are '-'
constexpr u64 GC_GAPS = 0x2D2D2D2D2D2D2D2Dull;         // eight '-'
template <bool VARIABLE, bool PARTIAL = false>
__global__ __launch_bounds__(GC_THREADS) void k_concat_text(const uint8_t *__restrict__ text, u64 text_bytes, const u64 *__restrict__ roff,
                                                            const u64 *__restrict__ first, u64 nused, const GcPick *__restrict__ picks,
                                                            const u64 *__restrict__ coff, unsigned nclass, const char *__restrict__ hdr,
                                                            u64 C, u64 S, unsigned width, u64 total, uint4 *__restrict__ out)
{
	__shared__ u64 s_off[GM_MAX_CLASS + 1];
	__shared__ unsigned s_first, s_last;
	const u64 span0 = (u64)blockIdx.x * GC_SPAN;
	if (span0 >= total) return;
	const u64 span1 = span0 + GC_SPAN < total ? span0 + GC_SPAN : total;      // one past the last byte of text in the span
	if (threadIdx.x == 0) s_first = bs_find(coff, nclass, span0);
	if (threadIdx.x == 1) s_last = bs_find(coff, nclass, span1 - 1);
	__syncthreads();
	const unsigned f0 = s_first, count = s_last - f0 + 1;                     // the classes whose rows the span touches
	for (unsigned i = threadIdx.x; i <= count; i += GC_THREADS) s_off[i] = coff[f0 + i];
	__syncthreads();

	const u64 t0 = span0 + (u64)threadIdx.x * 16;
	if (t0 >= span1) return;
	unsigned fi = bs_find(s_off, count, t0);                                  // the class row, counted from f0: never an empty one
	u64 off = t0 - s_off[fi], rlen = s_off[fi + 1] - s_off[fi], hlen = rlen - S;
	const u64 line = (u64)width + 1;
	unsigned col = 0;                                                         // place in the line ...
	u64 c = 0, g = 0;                                                         // ... the kept column the text goes on with and (ALL) its used group
	if (off >= hlen) { const u64 q = off - hlen; col = (unsigned)(q % line); c = q / line * width + col; }      // the one division of the lane
	B16 w;
	bool fast = false;
	if (!VARIABLE && off >= hlen && off + 16 <= rlen && width >= 16) {
		// 16 bytes of one class's sequence.  A line is width + 1 >= 17 bytes: at most one line feed of a full line in the piece, and
		// perhaps the one after the last column
		const unsigned full = width - col;                                    // col == width: the piece starts on the line feed
		const u64 last = rlen - 1 - off;                                      // >= 15
		unsigned nl = 16;                                                     // where a line feed falls in the piece (16: nowhere)
		fast = !(full < 16 && last < 16 && full != last);                     // both: a last line of a few columns
		if (fast) {
			nl = full < 16 ? full : last < 16 ? (unsigned)last : 16;
			g = bs_find(first, nused, c);                                     // c < C: the piece holds 15 columns at least
			fast = c + (nl < 16 ? 15 : 16) <= first[g + 1];                   // all of them in one group's row
		}
		if (fast) {
			const u64 r = roff[g * nclass + f0 + fi];
			w = PARTIAL && r == ~0ull ? B16{GC_GAPS, GC_GAPS} : gv_load16(text, text_bytes, r + (c - first[g]));
			if (nl < 16) w = insert_newline(w, nl);
		}
	}
	if (!fast) {
		// ---- headers, boundaries between class rows and between groups, narrow lines, picked columns: byte by byte, (c, col, g) stepped
		if (!VARIABLE && off >= hlen && c < C) g = bs_find(first, nused, c);
		w.lo = w.hi = 0;
		for (unsigned j = 0; j < 16 && t0 + j < total; j++) {
			while (off == rlen) { fi++; off = 0; rlen = s_off[fi + 1] - s_off[fi]; hlen = rlen - S; col = 0; c = 0; g = 0; }      // the next class row, from its start
			const u64 f = f0 + fi;
			unsigned char ch;
			if (off < hlen) ch = (unsigned char)hdr[s_off[fi] - f * S + off];
			else if (off + 1 == rlen || col == width) { ch = '\n'; col = 0; }
			else {
				u64 r, at;
				if (VARIABLE) { const GcPick p = picks[c]; r = roff[p.ug * nclass + f]; at = p.col; }
				else { while (c >= first[g + 1]) g++; r = roff[g * nclass + f]; at = c - first[g]; }
				ch = PARTIAL && r == ~0ull ? '-' : text[r + at];
				c++; col++;
			}
			if (j < 8) w.lo |= (u64)ch << (8 * j); else w.hi |= (u64)ch << (8 * (j - 8));
			off++;
		}
	}
	store16(out, t0 / 16, w);
}

}  // namespace

extern "C" sbl_status sbl_group_concat(sbl_ctx *c, const uint8_t *want, const uint32_t *cls, uint32_t nclass, uint32_t mode, uint32_t width,
                                       const char *headers, const uint64_t *header_first,
                                       const sbl_concat_part **parts, uint64_t *nparts, const sbl_concat_site **sites, uint64_t *nsites,
                                       const char **text, uint64_t *text_len)
{
	return guarded(c, [&] {
		require_group_rows(c);
		const uint8_t *const rows = gm_reader_rows(c);
		check_classes(c, cls, nclass);
		SBL_CHECK(mode == SBL_CONCAT_ALL || mode == SBL_CONCAT_VARIABLE, SBL_ERR_BAD_ARG, "unknown mode of concatenation");
		SBL_CHECK(width >= 1, SBL_ERR_BAD_ARG, "the width of a line must be at least 1");
		SBL_CHECK(headers && header_first, SBL_ERR_BAD_ARG, "null headers");
		for (uint32_t f = 0; f < nclass; f++) SBL_CHECK(header_first[f] <= header_first[f + 1], SBL_ERR_BAD_ARG, "descending header offsets");
		const bool variable = mode == SBL_CONCAT_VARIABLE, partial = c->gp_partial != 0;
		hipStream_t s = c->stream;
		c->gc_parts.clear(); c->gc_sites.clear();
		c->gc_times = SblTimes{};
		// the used groups -- one row is enough where there is one class --, where the row of every class starts and the parts of mode ALL;
		// with VARIABLE the used groups and the padded prefix of their columns go up (d_gm_used, d_gm_cbase)
		std::vector<u64> roff, first;
		const GmColumns cols = gm_class_columns(c, want, cls, nclass, variable, roff, first);
		const std::vector<GmUsed> &groups = cols.used;
		const u64 ng = groups.size(), P = cols.cbase.back(), text_bytes = cols.text_bytes;
		u64 C = variable ? 0 : first.back();
		float kernel_ms = 0;
		if (variable && ng) {
			// ---- the kept columns, ascending, and their number
			c->d_gc_flag.ensure((size_t)P); c->d_gc_x.ensure((size_t)P * 8); c->d_gm_count.ensure(16);
			HIP_TRY(hipEventRecord(c->ev[0], s));
			(partial ? k_site_flags<false, true> : k_site_flags<false, false>)<<<gm_blocks(P / 16), GC_THREADS, 0, s>>>(
				rows, text_bytes, c->d_gm_group.as<GmGroup>(), c->d_gm_used.as<GmUsed>(), c->d_gm_cbase.as<u64>(), ng, P, nclass, c->d_gc_flag.as<uint4>());
			HIP_TRY(hipGetLastError());
			prim::select(s, c->d_gm_tmp, rocprim::counting_iterator<u64>(0), c->d_gc_flag.as<uint8_t>(), c->d_gc_x.as<u64>(), c->d_gm_count.as<u64>(), (size_t)P);
			HIP_TRY(hipEventRecord(c->ev[1], s));
			HIP_TRY(hipMemcpyAsync(&C, c->d_gm_count.p, 8, hipMemcpyDeviceToHost, s));
			HIP_TRY(hipStreamSynchronize(s));
			kernel_ms = sbl_elapsed_ms(c, 0, 1);
		}
		// ---- the text: nclass rows of header and st_text_len(C, width) bytes
		const u64 S = st_text_len(C, width), h0 = header_first[0];
		std::vector<u64> coff(nclass + 1, 0);
		for (uint32_t f = 0; f < nclass; f++) coff[f + 1] = coff[f] + (header_first[f + 1] - header_first[f]) + S;
		const u64 total = coff[nclass];
		const size_t padded = (size_t)((total + 15) / 16 * 16);
		SBL_CHECK((total + GC_SPAN - 1) / GC_SPAN < 0x7FFFFFFFull, SBL_ERR_TOO_LARGE, "concatenated alignment too large");
		if (total) {
			const size_t hbytes = (size_t)(header_first[nclass] - h0);
			al_upload(c, c->d_gc_roff, roff); al_upload(c, c->d_gc_coff, coff);
			if (!variable) al_upload(c, c->d_gc_first, first);
			c->d_gc_hdr.ensure(std::max<size_t>(1, hbytes));
			if (hbytes) HIP_TRY(hipMemcpyAsync(c->d_gc_hdr.p, headers + h0, hbytes, hipMemcpyHostToDevice, s));
			c->d_gc_text.ensure(padded);
			c->d_gc_site.ensure(std::max<size_t>(1, (size_t)(variable ? C : 0)) * sizeof(sbl_concat_site));
			c->d_gc_pick.ensure(std::max<size_t>(1, (size_t)(variable ? C : 0)) * sizeof(GcPick));
			c->h_gc_text.ensure(padded, "host buffer for the concatenated alignment");
			if (variable) c->gc_sites.resize((size_t)C);
			const unsigned blocks = (unsigned)((total + GC_SPAN - 1) / GC_SPAN);
			HIP_TRY(hipEventRecord(c->ev[2], s));
			if (variable) {
				if (C) {
					k_site_fill<<<gm_blocks(C), GC_THREADS, 0, s>>>(c->d_gm_group.as<GmGroup>(), c->d_gm_slot.as<GmSlot>(), c->d_gm_used.as<GmUsed>(), c->d_gm_cbase.as<u64>(), ng,
					                                                c->d_gc_x.as<u64>(), C, c->d_gc_site.as<sbl_concat_site>(), c->d_gc_pick.as<GcPick>());
					HIP_TRY(hipGetLastError());
				}
				(partial ? k_concat_text<true, true> : k_concat_text<true, false>)<<<blocks, GC_THREADS, 0, s>>>(
					rows, text_bytes, c->d_gc_roff.as<u64>(), nullptr, ng, c->d_gc_pick.as<GcPick>(), c->d_gc_coff.as<u64>(), nclass, c->d_gc_hdr.as<char>(), C, S, width, total,
					c->d_gc_text.as<uint4>());
			} else
				(partial ? k_concat_text<false, true> : k_concat_text<false, false>)<<<blocks, GC_THREADS, 0, s>>>(
					rows, text_bytes, c->d_gc_roff.as<u64>(), c->d_gc_first.as<u64>(), ng, nullptr, c->d_gc_coff.as<u64>(), nclass, c->d_gc_hdr.as<char>(), C, S, width, total,
					c->d_gc_text.as<uint4>());
			HIP_TRY(hipGetLastError());
			HIP_TRY(hipEventRecord(c->ev[3], s));
			HIP_TRY(hipMemcpyAsync(c->h_gc_text.p, c->d_gc_text.p, padded, hipMemcpyDeviceToHost, s));
			HIP_TRY(hipEventRecord(c->ev[4], s));
			if (variable && C) HIP_TRY(hipMemcpyAsync(c->gc_sites.data(), c->d_gc_site.p, (size_t)C * sizeof(sbl_concat_site), hipMemcpyDeviceToHost, s));
			HIP_TRY(hipStreamSynchronize(s));
			kernel_ms += sbl_elapsed_ms(c, 2, 3);
			c->gc_times.copy_ms = sbl_elapsed_ms(c, 3, 4);
		}
		c->gc_times.kernel_ms = kernel_ms;
		// ---- the parts: in mode VARIABLE the sites of every used group, counted here (they come in ascending group)
		c->gc_parts.resize((size_t)ng);
		size_t at = 0;
		for (size_t u = 0; u < ng; u++) {
			u64 n = first[u + 1] - first[u];
			if (variable) { const size_t from = at; while (at < c->gc_sites.size() && c->gc_sites[at].group == groups[u].group) at++; n = at - from; }
			c->gc_parts[u] = sbl_concat_part{groups[u].group, u ? c->gc_parts[u - 1].first + c->gc_parts[u - 1].ncols : 0, n};
		}
		c->stats.device_bytes = sbl_devbuf_total().load();
		if (parts) *parts = c->gc_parts.data();
		if (nparts) *nparts = ng;
		if (sites) *sites = c->gc_sites.data();
		if (nsites) *nsites = c->gc_sites.size();
		if (text) *text = total ? c->h_gc_text.p : "";
		if (text_len) *text_len = total;
	});
}

extern "C" sbl_status sbl_group_set_partial(sbl_ctx *c, uint32_t on)
{
	return guarded(c, [&] {
		SBL_CHECK(on <= 1, SBL_ERR_BAD_ARG, "the partial groups setting is 0 or 1");
		c->gp_partial = on;
	});
}

extern "C" sbl_status sbl_group_get_partial(const sbl_ctx *c, uint32_t *on)
{
	if (!c || !on) return SBL_ERR_BAD_ARG;
	*on = c->gp_partial;
	return SBL_OK;
}

extern "C" sbl_status sbl_group_concat_times(const sbl_ctx *c, double *kernel_ms, double *copyback_ms)
{
	return sbl_times_out(c, &sbl_ctx::gc_times, kernel_ms, copyback_ms);
}
