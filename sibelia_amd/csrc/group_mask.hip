// group_mask.hip -- the SNP-density mask of the multiple alignments (include/sibelia_amd.h): per member row of the used
// groups of the last sbl_align_groups / sbl_align_block_groups call the maximal intervals in which more than max_diff differences from
// the centre row fall into `window` consecutive centre bases, and the rows with every byte other than '-' inside an interval replaced
// by N, in a buffer of the layout of the rows (d_gk_text) that sbl_group_variants, sbl_group_distances and sbl_group_concat read instead
// of the rows under sbl_group_set_masked.  The comparisons follow the bases (every column of every member row) and the rows are
// rewritten, so both run where the rows are; only the intervals come back.  Every pass is output-stationary.
//
//   flags     k_diff_flags.  Every member row of every used group padded to a multiple of 16 columns, in ONE flat index space: used group
//             u starts at rbase[u], the prefix of (r - 1) * padded L, uploaded next to gm_columns' tables.  A lane owns 16 columns of ONE
//             member row: the centre's and the row's 16 bytes (gv_load16), base_flags8(centre) & base_flags8(row) & nonzero8(centre ^
//             row), the tail cut (keep16), 16 flag bytes in one vector store.  Padding gets 0.
//   select    rocPRIM's select over a counting iterator: the D flat indices of the differences, ascending = by (group, row, column).
//             The host reads D, the first of two count reads; D == 0 ends with a plain copy of the rows.
//   fill      k_diff_fill, one lane per difference: (used group, row, column) by bs_find over rbase and one division by the padded L;
//             the centre index from the merged gap slots (gm_centre_before).  It writes a key that is one number per member row of the
//             call (used group << 32 | row), the centre index and the column.
//   starts    k_dense_start, one lane per difference j: s_j = (j + T < D && key[j + T] == key[j] && pos[j + T] - pos[j] < W), in 64-bit
//             arithmetic; an exclusive scan of s (D + 1 values, s_D = 0), so that "no start among the T differences before / after" is
//             one subtraction and the cost does not follow T.  k_dense_ends: a head is a start j with no start in [j - T, j); a tail is
//             difference k + T of a start k with no start in (k, k + T].  The j-th head pairs with the j-th tail.  Two selects compact
//             them; the host reads their number M, the second count read.
//   intervals k_mask_fill, one lane per interval: the sbl_mask_interval and its flat byte range [a, b] in the rows.  The ranges are
//             ascending and disjoint (the groups lie in d_ga_text in order, their rows one after the other).
//   rows      k_mask_rows.  A lane owns 16 aligned bytes of the rows text -- row starts are not aligned: its word may hold the end of
//             one row and the start of the next, for short rows several rows and several intervals.  It finds the first interval with
//             b >= its first byte by binary search over the ends, applies every interval that starts at or before its last byte to the
//             bytes other than '-' and writes one 16-byte store.  Bytes of unused groups meet no interval: they are copied.
//   host      every argument is checked before any launch; the used groups by the walk of sbl_groups.h (gm_columns, two rows at least);
//             event pairs around the kernels and around the copy of the intervals; the workspace of the compactions is sized once per
//             phase, before its first launch.
#include <algorithm>
#include <cstring>

#include "sbl_groups.h"
#include "sbl_prim.h"

namespace {

constexpr unsigned GK_THREADS = GM_THREADS;
constexpr u64 GK_GAPS = 0x2D2D2D2D2D2D2D2Dull, GK_NS = 0x4E4E4E4E4E4E4E4Eull;

// the member row and the column of flat index y of a used group of padded length PL: row >= 1
struct GkPlace { u64 row, col; };
__device__ inline GkPlace gk_place(u64 y, u64 PL) { const u64 q = y / PL; return {q + 1, y - q * PL}; }

__global__ __launch_bounds__(GK_THREADS) void k_diff_flags(const uint8_t *__restrict__ text, u64 text_bytes, const GmGroup *__restrict__ gm,
                                                           const GmUsed *__restrict__ used, const u64 *__restrict__ cbase, const u64 *__restrict__ rbase,
                                                           u64 nused, u64 flat, uint4 *__restrict__ flags)
{
	const u64 x0 = ((u64)blockIdx.x * GK_THREADS + threadIdx.x) * 16;
	if (x0 >= flat) return;
	const unsigned gi = bs_find(rbase, nused, x0);
	const GmGroup Q = gm[used[gi].dg];
	const GkPlace at = gk_place(x0 - rbase[gi], cbase[gi + 1] - cbase[gi]);      // at.col < L: the padding of a row is less than 16 columns
	const unsigned n = Q.L - at.col < 16 ? (unsigned)(Q.L - at.col) : 16;
	const B16 ref = gv_load16(text, text_bytes, Q.toff + at.col);
	const B16 w = gv_load16(text, text_bytes, Q.toff + at.row * Q.L + at.col);
	B16 o = {(base_flags8(ref.lo) & base_flags8(w.lo) & nonzero8(ref.lo ^ w.lo)) >> 7, (base_flags8(ref.hi) & base_flags8(w.hi) & nonzero8(ref.hi ^ w.hi)) >> 7};
	if (n < 16) o = keep16(o, n, 0);
	store16(flags, x0 / 16, o);
}

__global__ __launch_bounds__(GK_THREADS) void k_diff_fill(const GmGroup *__restrict__ gm, const GmSlot *__restrict__ slots, const GmUsed *__restrict__ used,
                                                          const u64 *__restrict__ cbase, const u64 *__restrict__ rbase, u64 nused,
                                                          const u64 *__restrict__ xs, u64 D, u64 *__restrict__ key, u64 *__restrict__ pos, u64 *__restrict__ col)
{
	const u64 i = (u64)blockIdx.x * GK_THREADS + threadIdx.x;
	if (i >= D) return;
	const u64 x = xs[i];
	const unsigned gi = bs_find(rbase, nused, x);
	const GmGroup Q = gm[used[gi].dg];
	const GkPlace at = gk_place(x - rbase[gi], cbase[gi + 1] - cbase[gi]);
	key[i] = ((u64)gi << 32) | at.row;
	pos[i] = gm_centre_before(slots, Q, at.col);
	col[i] = at.col;
}

// s[0 .. D]: s[j] = difference j starts a dense run; s[D] = 0
__global__ __launch_bounds__(GK_THREADS) void k_dense_start(const u64 *__restrict__ key, const u64 *__restrict__ pos, u64 D, u64 W, u64 T, u64 *__restrict__ s)
{
	const u64 j = (u64)blockIdx.x * GK_THREADS + threadIdx.x;
	if (j > D) return;
	const u64 e = j + T;                                                      // T < 2^32, j < 2^63: no wrap
	s[j] = j < D && e < D && key[e] == key[j] && pos[e] - pos[j] < W;
}

// E[0 .. D]: the starts in [0, j).  head[j]: j is a start and none of the T differences before it is; tail[j]: j - T is a start and none
// of the T differences after THAT is
__global__ __launch_bounds__(GK_THREADS) void k_dense_ends(const u64 *__restrict__ s, const u64 *__restrict__ E, u64 D, u64 T,
                                                           uint8_t *__restrict__ head, uint8_t *__restrict__ tail)
{
	const u64 j = (u64)blockIdx.x * GK_THREADS + threadIdx.x;
	if (j >= D) return;
	const u64 ej = E[j];
	head[j] = s[j] && ej == E[j > T ? j - T : 0];
	tail[j] = j >= T && s[j - T] && E[j + 1] == E[j - T + 1];
}

__global__ __launch_bounds__(GK_THREADS) void k_mask_fill(const GmGroup *__restrict__ gm, const GmUsed *__restrict__ used, const u64 *__restrict__ key,
                                                          const u64 *__restrict__ pos, const u64 *__restrict__ col, const u64 *__restrict__ heads,
                                                          const u64 *__restrict__ tails, u64 M, sbl_mask_interval *__restrict__ iv,
                                                          u64 *__restrict__ ra, u64 *__restrict__ rb)
{
	const u64 m = (u64)blockIdx.x * GK_THREADS + threadIdx.x;
	if (m >= M) return;
	const u64 h = heads[m], t = tails[m], k = key[h], row = k & 0xFFFFFFFFull;
	const GmUsed U = used[k >> 32];
	const GmGroup Q = gm[U.dg];
	iv[m] = sbl_mask_interval{U.group, row, col[h], col[t], pos[h], pos[t], t - h + 1};
	const u64 base = Q.toff + row * Q.L;
	ra[m] = base + col[h];
	rb[m] = base + col[t];
}

// 0xFF in bytes [lo, hi] of a 64-bit word, 0 <= lo <= hi <= 7
__device__ inline u64 gk_range8(unsigned lo, unsigned hi) { return (~0ull >> (8 * (7 - hi))) & (~0ull << (8 * lo)); }
// v with its bytes other than '-' in the bytes `sel` selects (0xFF each) replaced by 'N'
__device__ inline u64 gk_mask8(u64 v, u64 sel)
{
	const u64 take = sel & ((nonzero8(v ^ GK_GAPS) >> 7) * 0xFF);
	return (v & ~take) | (GK_NS & take);
}

__global__ __launch_bounds__(GK_THREADS) void k_mask_rows(const uint4 *__restrict__ text, u64 text_bytes, const u64 *__restrict__ ra, const u64 *__restrict__ rb, u64 M,
                                                          uint4 *__restrict__ out)
{
	const u64 t0 = ((u64)blockIdx.x * GK_THREADS + threadIdx.x) * 16;
	if (t0 >= text_bytes) return;
	const uint4 v = text[t0 / 16];
	B16 w = {(u64)v.x | ((u64)v.y << 32), (u64)v.z | ((u64)v.w << 32)};
	u64 lo = 0, hi = M;                                                       // the first interval that ends at or behind t0
	while (lo < hi) {
		const u64 mid = lo + (hi - lo) / 2;
		if (rb[mid] < t0) lo = mid + 1; else hi = mid;
	}
	for (u64 m = lo; m < M; m++) {
		const u64 a = ra[m];
		if (a > t0 + 15) break;
		const u64 b = rb[m];
		const unsigned from = a > t0 ? (unsigned)(a - t0) : 0, to = b < t0 + 15 ? (unsigned)(b - t0) : 15;
		if (from < 8) w.lo = gk_mask8(w.lo, gk_range8(from, to < 8 ? to : 7));
		if (to >= 8) w.hi = gk_mask8(w.hi, gk_range8(from > 8 ? from - 8 : 0, to - 8));
	}
	store16(out, t0 / 16, w);
}

}  // namespace

extern "C" sbl_status sbl_group_mask(sbl_ctx *c, const uint8_t *want, uint32_t window, uint32_t max_diff, const sbl_mask_interval **intervals, uint64_t *nintervals)
{
	return guarded(c, [&] {
		require_group_rows(c);
		SBL_CHECK(window >= 1, SBL_ERR_BAD_ARG, "the window of the density mask must be at least 1");
		SBL_CHECK(max_diff >= 1, SBL_ERR_BAD_ARG, "the differences a window may hold must be at least 1");
		hipStream_t s = c->stream;
		const u64 W = window, T = max_diff;
		// the used groups -- two rows at least --, checked and up (d_gm_used, d_gm_cbase), and the prefix of their padded member rows
		std::vector<u64> rbase(1, 0);
		const GmColumns cols = gm_columns(c, want, 2, true, [&](size_t, const sbl_group_result &r, u64) {
			rbase.push_back(rbase.back() + (u64)(r.ninst - 1) * ((r.L + 15) / 16 * 16));
		});
		const u64 ng = cols.used.size(), F = rbase.back(), text_bytes = cols.text_bytes;
		SBL_CHECK(!text_bytes || (c->d_ga_text.p && c->d_ga_text.cap >= text_bytes), SBL_ERR_INTERNAL, "the rows of the groups are not on the device");
		const unsigned flag_blocks = gm_blocks(F / 16), text_blocks = gm_blocks(text_bytes / 16);      // every grid that does not follow a count, before any launch
		c->gk_valid = false;
		c->gk_intervals.clear();
		c->gk_times = SblTimes{};
		c->d_gk_text.ensure(std::max<size_t>(16, (size_t)text_bytes));
		const GmGroup *const gm = c->d_gm_group.as<GmGroup>();
		const GmUsed *const used = c->d_gm_used.as<GmUsed>();
		const u64 *const cbase = c->d_gm_cbase.as<u64>();
		u64 D = 0, M = 0;
		float kernel_ms = 0;
		if (ng) {
			// ---- the differences, ascending, and their number
			al_upload(c, c->d_gk_rbase, rbase);
			c->d_gk_flag.ensure((size_t)F); c->d_gk_x.ensure((size_t)F * 8); c->d_gm_count.ensure(16);
			HIP_TRY(hipEventRecord(c->ev[0], s));
			k_diff_flags<<<flag_blocks, GK_THREADS, 0, s>>>(c->d_ga_text.as<uint8_t>(), text_bytes, gm, used, cbase, c->d_gk_rbase.as<u64>(), ng, F, c->d_gk_flag.as<uint4>());
			HIP_TRY(hipGetLastError());
			prim::select(s, c->d_gm_tmp, rocprim::counting_iterator<u64>(0), c->d_gk_flag.as<uint8_t>(), c->d_gk_x.as<u64>(), c->d_gm_count.as<u64>(), (size_t)F);
			HIP_TRY(hipEventRecord(c->ev[1], s));
			HIP_TRY(hipMemcpyAsync(&D, c->d_gm_count.p, 8, hipMemcpyDeviceToHost, s));
			HIP_TRY(hipStreamSynchronize(s));
			kernel_ms = sbl_elapsed_ms(c, 0, 1);
		}
		if (D) {
			// ---- place of every difference, the starts of dense runs, their scan, heads and tails and their number
			c->d_gk_diff.ensure((size_t)D * 24); c->d_gk_start.ensure((size_t)(D + 1) * 8); c->d_gk_scan.ensure((size_t)(D + 1) * 8);
			c->d_gk_end.ensure((size_t)D * 2); c->d_gk_head.ensure((size_t)D * 8); c->d_gk_tail.ensure((size_t)D * 8);
			u64 *const key = c->d_gk_diff.as<u64>(), *const pos = key + D, *const col = pos + D;
			u64 *const st = c->d_gk_start.as<u64>(), *const E = c->d_gk_scan.as<u64>();
			uint8_t *const f_head = c->d_gk_end.as<uint8_t>(), *const f_tail = f_head + D;
			u64 *const cnt = c->d_gm_count.as<u64>();
			const unsigned blocks = gm_blocks(D + 1);
			const rocprim::counting_iterator<u64> ids(0);
			c->d_gm_tmp.ensure(std::max(prim::query([&](void *t, size_t &b) { return rocprim::exclusive_scan(t, b, st, E, 0ull, (size_t)(D + 1), rocprim::plus<u64>(), s); }),
			                            prim::query([&](void *t, size_t &b) { return rocprim::select(t, b, ids, f_head, c->d_gk_head.as<u64>(), cnt, (size_t)D, s); })));
			u64 count[2] = {0, 0};
			HIP_TRY(hipEventRecord(c->ev[2], s));
			k_diff_fill<<<gm_blocks(D), GK_THREADS, 0, s>>>(gm, c->d_gm_slot.as<GmSlot>(), used, cbase, c->d_gk_rbase.as<u64>(), ng, c->d_gk_x.as<u64>(), D, key, pos, col);
			HIP_TRY(hipGetLastError());
			k_dense_start<<<blocks, GK_THREADS, 0, s>>>(key, pos, D, W, T, st);
			HIP_TRY(hipGetLastError());
			prim::exclusive_scan(s, c->d_gm_tmp, st, E, 0ull, (size_t)(D + 1), rocprim::plus<u64>());
			k_dense_ends<<<gm_blocks(D), GK_THREADS, 0, s>>>(st, E, D, T, f_head, f_tail);
			HIP_TRY(hipGetLastError());
			prim::select(s, c->d_gm_tmp, ids, f_head, c->d_gk_head.as<u64>(), cnt, (size_t)D);
			prim::select(s, c->d_gm_tmp, ids, f_tail, c->d_gk_tail.as<u64>(), cnt + 1, (size_t)D);
			HIP_TRY(hipEventRecord(c->ev[3], s));
			HIP_TRY(hipMemcpyAsync(count, c->d_gm_count.p, 16, hipMemcpyDeviceToHost, s));
			HIP_TRY(hipStreamSynchronize(s));
			kernel_ms += sbl_elapsed_ms(c, 2, 3);
			SBL_CHECK(count[0] == count[1], SBL_ERR_INTERNAL, "the dense runs of the alignments do not close");
			M = count[0];
		}
		if (M) {
			// ---- the intervals, their byte ranges and the masked rows
			c->d_gk_iv.ensure((size_t)M * sizeof(sbl_mask_interval)); c->d_gk_range.ensure((size_t)M * 16);
			c->gk_intervals.resize((size_t)M);
			u64 *const key = c->d_gk_diff.as<u64>(), *const pos = key + D, *const col = pos + D;
			u64 *const ra = c->d_gk_range.as<u64>(), *const rb = ra + M;
			HIP_TRY(hipEventRecord(c->ev[4], s));
			k_mask_fill<<<gm_blocks(M), GK_THREADS, 0, s>>>(gm, used, key, pos, col, c->d_gk_head.as<u64>(), c->d_gk_tail.as<u64>(), M, c->d_gk_iv.as<sbl_mask_interval>(), ra, rb);
			HIP_TRY(hipGetLastError());
			k_mask_rows<<<text_blocks, GK_THREADS, 0, s>>>(c->d_ga_text.as<uint4>(), text_bytes, ra, rb, M, c->d_gk_text.as<uint4>());
			HIP_TRY(hipGetLastError());
			HIP_TRY(hipEventRecord(c->ev[5], s));
			HIP_TRY(hipMemcpyAsync(c->gk_intervals.data(), c->d_gk_iv.p, (size_t)M * sizeof(sbl_mask_interval), hipMemcpyDeviceToHost, s));
			HIP_TRY(hipEventRecord(c->ev[6], s));
			HIP_TRY(hipStreamSynchronize(s));
			kernel_ms += sbl_elapsed_ms(c, 4, 5);
			c->gk_times.copy_ms = sbl_elapsed_ms(c, 5, 6);
		} else if (text_bytes) {
			// ---- no difference or no interval: the masked rows are the rows
			HIP_TRY(hipEventRecord(c->ev[4], s));
			HIP_TRY(hipMemcpyAsync(c->d_gk_text.p, c->d_ga_text.p, (size_t)text_bytes, hipMemcpyDeviceToDevice, s));
			HIP_TRY(hipEventRecord(c->ev[5], s));
			HIP_TRY(hipStreamSynchronize(s));
			kernel_ms += sbl_elapsed_ms(c, 4, 5);
		}
		c->gk_times.kernel_ms = kernel_ms;
		c->gk_valid = true;
		c->stats.device_bytes = sbl_devbuf_total().load();
		if (intervals) *intervals = c->gk_intervals.data();
		if (nintervals) *nintervals = M;
	});
}

extern "C" sbl_status sbl_group_mask_times(const sbl_ctx *c, double *kernel_ms, double *copyback_ms)
{
	return sbl_times_out(c, &sbl_ctx::gk_times, kernel_ms, copyback_ms);
}

extern "C" sbl_status sbl_group_set_masked(sbl_ctx *c, uint32_t on)
{
	return guarded(c, [&] {
		SBL_CHECK(on <= 1, SBL_ERR_BAD_ARG, "the masked rows setting is 0 or 1");
		c->gk_masked = on;
	});
}

extern "C" sbl_status sbl_group_get_masked(const sbl_ctx *c, uint32_t *on)
{
	if (!c || !on) return SBL_ERR_BAD_ARG;
	*on = c->gk_masked;
	return SBL_OK;
}
