// group_variants.hip -- the variant segments of the multiple alignments (include/sibelia_amd.h): the N-row form of the
// rules parse_alignment (reference src/csibelia/C-Sibelia.py:206-252) applies to the two rows of a pair, on the rows the last
// sbl_align_groups / sbl_align_block_groups call left on the device (d_ga_text, spelled by k_spell_groups through d_gm_group / d_gm_slot).
// The rows hold as many bytes as the blocks have bases times instances; the segments follow the edits.  So the column-wise pass runs
// where the rows are and only the segments and their slices come back.
//
//   classes   k_column_classes, the column walk of sbl_groups.h (gm_walk16: a lane owns 16 consecutive columns of ONE group, every group
//             padded to a multiple of 16 columns) with "any row holds '-'" gathered next to "differs from row 0": 16 class bytes per
//             lane, 0 equal, 1 unequal, 3 unequal and gapped.
//   bounds    k_segment_bounds, one lane per column: an unequal column OPENS a segment if it is column 0 or the equal run that ends before
//             it is kept, and CLOSES one if it is column L - 1 or the equal run that starts behind it is kept.  "Kept" (the run touches
//             column 0 or L, or has 30 columns) is decided by looking at most 30 class bytes back / ahead.  The lane writes two flag
//             bytes; the flagged columns are compacted in ascending order by rocPRIM's select (sbl_prim.h), opens and closes apart.
//   segments  k_segment_fill, one lane per segment: the i-th open pairs with the i-th close; lead, `before` from the group's merged gap
//             slots (gm_centre_before) and where its slices lie in the rows.  k_segment_gapped, one lane per column: a gapped column
//             finds its segment by binary search over the opens and marks it.
//   slices    k_gather_slices, output-stationary like k_spell_groups: a lane owns 16 bytes of the packed text, finds its segment by
//             binary search over the text offsets, then row and column; 16 bytes inside one slice are cut out of two aligned words,
//             everything else steps byte by byte.  One vector store per lane.
//   host      the group table and the 64-bit prefix of the padded L (gm_columns, sbl_groups.h) and, between the launches, the two counts
//             and the prefix of the slice lengths (their number follows the edits).  The slices come back into a buffer of their own.
#include <algorithm>
#include <cstring>

#include "sbl_groups.h"
#include "sbl_prim.h"

namespace {

constexpr unsigned GV_THREADS = GM_THREADS;
constexpr unsigned GV_CONTEXT = 30;                    // MINIMUM_CONTEXT_SIZE (C-Sibelia.py:20)
constexpr u64 GV_GAPS = 0x2D2D2D2D2D2D2D2Dull;         // '-'

struct GvSlice { u64 src, L, len; };                   // a segment's slices: first byte of the centre's in the rows, row stride, bytes per row

// gm_walk16's reader of the classes: 0x80 in every byte whose column holds a '-' in any of the group's rows
struct GvClasses {
	u64 glo, ghi;
	__device__ unsigned rows(const GmGroup &Q) const { return Q.ninst; }
	__device__ void first(B16 ref) { glo = zero8(ref.lo ^ GV_GAPS); ghi = zero8(ref.hi ^ GV_GAPS); }
	__device__ void next(B16 w) { glo |= zero8(w.lo ^ GV_GAPS); ghi |= zero8(w.hi ^ GV_GAPS); }
	__device__ B16 bytes(u64 ulo, u64 uhi) const { return {(ulo >> 7) | ((ulo & glo) >> 6), (uhi >> 7) | ((uhi & ghi) >> 6)}; }
};

__global__ __launch_bounds__(GV_THREADS) void k_column_classes(const uint8_t *__restrict__ text, u64 text_bytes, const GmGroup *__restrict__ gm,
                                                               const GmUsed *__restrict__ groups, const u64 *__restrict__ cbase, u64 ngroups,
                                                               u64 padded_cols, uint4 *__restrict__ cls)
{
	gm_walk16(text, text_bytes, gm, groups, cbase, ngroups, padded_cols, GvClasses{}, cls);
}

__global__ __launch_bounds__(GV_THREADS) void k_segment_bounds(const uint8_t *__restrict__ cls, const GmGroup *__restrict__ gm, const GmUsed *__restrict__ groups,
                                                               const u64 *__restrict__ cbase, u64 ngroups, u64 padded_cols,
                                                               uint8_t *__restrict__ opens, uint8_t *__restrict__ closes)
{
	const u64 x = (u64)blockIdx.x * GV_THREADS + threadIdx.x;
	if (x >= padded_cols) return;
	const unsigned gi = bs_find(cbase, ngroups, x);
	const u64 L = gm[groups[gi].dg].L, c = x - cbase[gi];
	const uint8_t *const k = cls + cbase[gi];                                 // the group's class bytes
	uint8_t open = 0, close = 0;
	if (c < L && k[c]) {
		// the equal run that ends at column c - 1: kept if it reaches column 0 or has GV_CONTEXT columns
		u64 back = 0;
		while (back < GV_CONTEXT && back < c && !k[c - 1 - back]) back++;
		open = c == 0 || (back > 0 && (back == c || back == GV_CONTEXT));
		// the equal run that starts at column c + 1: kept if it reaches column L or has GV_CONTEXT columns
		const u64 room = L - 1 - c;
		u64 ahead = 0;
		while (ahead < GV_CONTEXT && ahead < room && !k[c + 1 + ahead]) ahead++;
		close = room == 0 || (ahead > 0 && (ahead == room || ahead == GV_CONTEXT));
	}
	opens[x] = open; closes[x] = close;
}

__global__ __launch_bounds__(GV_THREADS) void k_segment_fill(const uint8_t *__restrict__ cls, const GmGroup *__restrict__ gm, const GmSlot *__restrict__ slots,
                                                             const GmUsed *__restrict__ groups, const u64 *__restrict__ cbase, u64 ngroups,
                                                             const u64 *__restrict__ opens, const u64 *__restrict__ closes, u64 nsegs,
                                                             sbl_group_segment *__restrict__ segs, GvSlice *__restrict__ slices)
{
	const u64 i = (u64)blockIdx.x * GV_THREADS + threadIdx.x;
	if (i >= nsegs) return;
	const u64 x = opens[i];
	const unsigned gi = bs_find(cbase, ngroups, x);
	const GmGroup Q = gm[groups[gi].dg];
	const u64 s = x - cbase[gi], e = closes[i] + 1 - cbase[gi];
	const unsigned lead = s == 0 || (e - s == 1 && cls[x] == 1) ? 0u : 1u;
	segs[i] = sbl_group_segment{groups[gi].group, s, e, gm_centre_before(slots, Q, s), 0, lead, 0};
	slices[i] = GvSlice{Q.toff + s - lead, Q.L, e - s + lead};
}

__global__ __launch_bounds__(GV_THREADS) void k_segment_gapped(const uint8_t *__restrict__ cls, u64 padded_cols, const u64 *__restrict__ opens, u64 nsegs,
                                                               sbl_group_segment *__restrict__ segs)
{
	const u64 x = (u64)blockIdx.x * GV_THREADS + threadIdx.x;
	if (x >= padded_cols || cls[x] != 3) return;
	segs[bs_find(opens, nsegs, x)].gapped = 1;                                // every unequal column lies in a segment: opens[0] <= x
}

__global__ __launch_bounds__(GV_THREADS) void k_gather_slices(const uint8_t *__restrict__ text, u64 text_bytes, const GvSlice *__restrict__ slices,
                                                              const u64 *__restrict__ toff /* nsegs + 1 */, u64 nsegs, u64 total, uint4 *__restrict__ out)
{
	const u64 t0 = ((u64)blockIdx.x * GV_THREADS + threadIdx.x) * 16;
	if (t0 >= total) return;
	u64 si = bs_find(toff, nsegs, t0);
	GvSlice V = slices[si];
	u64 off = t0 - toff[si], row = off / V.len, k = off - row * V.len;       // a slice holds at least one byte
	B16 w;
	if (k + 16 <= V.len) w = gv_load16(text, text_bytes, V.src + row * V.L + k);
	else {
		w.lo = w.hi = 0;
		u64 end = toff[si + 1];
		for (unsigned b = 0; b < 16 && t0 + b < total; b++) {
			if (t0 + b == end) { si++; V = slices[si]; end = toff[si + 1]; row = 0; k = 0; }
			else if (k == V.len) { row++; k = 0; }
			const u64 ch = text[V.src + row * V.L + k];
			if (b < 8) w.lo |= ch << (8 * b); else w.hi |= ch << (8 * (b - 8));
			k++;
		}
	}
	store16(out, t0 / 16, w);
}

}  // namespace

extern "C" sbl_status sbl_group_variants(sbl_ctx *c, const uint8_t *want, const sbl_group_segment **segs, uint64_t *nsegs,
                                         const char **text, uint64_t *text_len)
{
	return guarded(c, [&] {
		require_group_rows(c);
		const uint8_t *const rows = gm_reader_rows(c);
		hipStream_t s = c->stream;
		c->gv_segs.clear(); c->gv_text.clear();
		c->gv_times = SblTimes{};
		// the wanted groups that have columns to compare, checked and up (d_gm_used, d_gm_cbase)
		const GmColumns cols = gm_columns(c, want, 2, true, [](size_t, const sbl_group_result &, u64) {});
		const u64 ng = cols.used.size(), P = cols.cbase.back(), text_bytes = cols.text_bytes;
		const GmUsed *const used = c->d_gm_used.as<GmUsed>();
		const u64 *const cbase = c->d_gm_cbase.as<u64>();
		u64 nseg = 0, total = 0;
		if (ng) {
			const GmGroup *gm = c->d_gm_group.as<GmGroup>();
			c->d_gv_class.ensure((size_t)P); c->d_gv_flag.ensure((size_t)(2 * P));
			c->d_gv_open.ensure((size_t)P * 8); c->d_gv_close.ensure((size_t)P * 8); c->d_gm_count.ensure(16);
			uint8_t *const f_open = c->d_gv_flag.as<uint8_t>(), *const f_close = f_open + P;
			u64 count[2] = {0, 0};
			HIP_TRY(hipEventRecord(c->ev[0], s));
			k_column_classes<<<gm_blocks(P / 16), GV_THREADS, 0, s>>>(rows, text_bytes, gm, used, cbase, ng, P, c->d_gv_class.as<uint4>());
			HIP_TRY(hipGetLastError());
			k_segment_bounds<<<gm_blocks(P), GV_THREADS, 0, s>>>(c->d_gv_class.as<uint8_t>(), gm, used, cbase, ng, P, f_open, f_close);
			HIP_TRY(hipGetLastError());
			prim::select(s, c->d_gm_tmp, rocprim::counting_iterator<u64>(0), f_open, c->d_gv_open.as<u64>(), c->d_gm_count.as<u64>(), (size_t)P);
			prim::select(s, c->d_gm_tmp, rocprim::counting_iterator<u64>(0), f_close, c->d_gv_close.as<u64>(), c->d_gm_count.as<u64>() + 1, (size_t)P);
			HIP_TRY(hipMemcpyAsync(count, c->d_gm_count.p, 16, hipMemcpyDeviceToHost, s));
			HIP_TRY(hipStreamSynchronize(s));
			SBL_CHECK(count[0] == count[1], SBL_ERR_INTERNAL, "the segments of the alignments do not close");
			nseg = count[0];
		}
		if (nseg) {
			c->d_gv_seg.ensure((size_t)nseg * sizeof(sbl_group_segment)); c->d_gv_slice.ensure((size_t)nseg * sizeof(GvSlice));
			c->gv_segs.resize((size_t)nseg);
			std::vector<GvSlice> slices((size_t)nseg);
			k_segment_fill<<<gm_blocks(nseg), GV_THREADS, 0, s>>>(c->d_gv_class.as<uint8_t>(), c->d_gm_group.as<GmGroup>(), c->d_gm_slot.as<GmSlot>(), used, cbase, ng,
			                                                      c->d_gv_open.as<u64>(), c->d_gv_close.as<u64>(), nseg, c->d_gv_seg.as<sbl_group_segment>(), c->d_gv_slice.as<GvSlice>());
			HIP_TRY(hipGetLastError());
			k_segment_gapped<<<gm_blocks(P), GV_THREADS, 0, s>>>(c->d_gv_class.as<uint8_t>(), P, c->d_gv_open.as<u64>(), nseg, c->d_gv_seg.as<sbl_group_segment>());
			HIP_TRY(hipGetLastError());
			HIP_TRY(hipEventRecord(c->ev[2], s));
			HIP_TRY(hipMemcpyAsync(c->gv_segs.data(), c->d_gv_seg.p, (size_t)nseg * sizeof(sbl_group_segment), hipMemcpyDeviceToHost, s));
			HIP_TRY(hipMemcpyAsync(slices.data(), c->d_gv_slice.p, (size_t)nseg * sizeof(GvSlice), hipMemcpyDeviceToHost, s));
			HIP_TRY(hipStreamSynchronize(s));
			// where the slices of every segment start in the packed text: ninst slices of `len` bytes each
			std::vector<u64> toff((size_t)nseg + 1, 0);
			for (size_t i = 0; i < nseg; i++) {
				sbl_group_segment &g = c->gv_segs[i];
				g.text_off = toff[i];
				toff[i + 1] = toff[i] + (u64)c->gm_res[g.group].ninst * slices[i].len;
			}
			total = toff.back();
			const size_t padded = (size_t)((total + 15) / 16 * 16);
			al_upload(c, c->d_gv_toff, toff);
			c->d_gv_text.ensure(padded);
			c->gv_text.resize(padded);
			HIP_TRY(hipEventRecord(c->ev[3], s));
			k_gather_slices<<<gm_blocks(padded / 16), GV_THREADS, 0, s>>>(rows, text_bytes, c->d_gv_slice.as<GvSlice>(), c->d_gv_toff.as<u64>(), nseg, total,
			                                                              c->d_gv_text.as<uint4>());
			HIP_TRY(hipGetLastError());
			HIP_TRY(hipEventRecord(c->ev[4], s));
			HIP_TRY(hipMemcpyAsync(c->gv_text.data(), c->d_gv_text.p, padded, hipMemcpyDeviceToHost, s));
			HIP_TRY(hipEventRecord(c->ev[5], s));
			HIP_TRY(hipStreamSynchronize(s));
			c->gv_times.kernel_ms = sbl_elapsed_ms(c, 0, 2) + sbl_elapsed_ms(c, 3, 4);      // the prefix of the slice lengths on the host lies between
			c->gv_times.copy_ms = sbl_elapsed_ms(c, 4, 5);
		} else if (ng) {
			HIP_TRY(hipEventRecord(c->ev[2], s));
			HIP_TRY(hipStreamSynchronize(s));
			c->gv_times.kernel_ms = sbl_elapsed_ms(c, 0, 2);
		}
		c->stats.device_bytes = sbl_devbuf_total().load();
		if (segs) *segs = c->gv_segs.data();
		if (nsegs) *nsegs = nseg;
		if (text) *text = total ? c->gv_text.data() : "";
		if (text_len) *text_len = total;
	});
}

extern "C" sbl_status sbl_group_variants_times(const sbl_ctx *c, double *kernel_ms, double *copyback_ms)
{
	return sbl_times_out(c, &sbl_ctx::gv_times, kernel_ms, copyback_ms);
}
