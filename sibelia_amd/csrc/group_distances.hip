// group_distances.hip -- the pairwise counts of the multiple alignments (include/sibelia_amd.h): for every ordered pair of
// rows of a group the columns that match, mismatch, are ambiguous or hold a gap in one of the two, summed into a matrix over the CLASSES
// the caller gives the instances (the pipeline: the input file), on the rows the last sbl_align_groups / sbl_align_block_groups call
// left on the device (d_ga_text).  A group of r rows asks for r (r - 1) / 2 row comparisons per column; the answer is nclass x nclass
// cells of four integers.  So the comparisons run where the rows are and only the matrix comes back.
//
//   items     the host cuts the work into items (wanted group, row block I, row block J >= I, span of columns): row blocks of at most
//             GD_ROWS = 32 rows; the columns of a group in spans so that the items of one call fill the card when the groups are few
//             and wide, and one span per group when they are many.  Their number follows groups and row blocks: the spans add at most
//             GD_TARGET items to a call.  An item carries the group's text offset and L from the host's gm_res (they equal d_gm_group's
//             toff and L), so the kernel has no dependent table load.
//   kernel    k_group_distances, one workgroup of 256 lanes per item, tile by tile (GD_TILE = 256 columns) over its span:
//     stage   the tile of both row blocks (of one, on the diagonal I == J) into LDS by aligned 16-byte loads shifted in registers
//             (gv_load16: toff + i L is not aligned in general).  Bytes behind the span's last column belong to the next span, the
//             next row or nothing: they are staged as '-' (keep16, sbl_groups.h), and a column of two gaps counts nowhere.  Next to the 8 bytes of a word the
//             lane stages their FLAGS, once per row and tile instead of once per pair: 0x80 in a byte that is one of A C G T, 0x40 in
//             a byte that is '-' (zero8).  The LDS row stride is 264 bytes: 66 dwords, so the 32 lanes of a half wave that read one
//             word of 32 different rows take 32 different bank pairs (a stride of 256 would be one bank for all).
//     sweep   lane t owns the pairs (i, j) = (t / 32 + 8 q, t % 32), q = 0 .. 3, of the block pair -- one row j and four rows i; on
//             the diagonal only i < j.  Per 8 columns it reads word and flags of row j once and of each row i (the 32 lanes of a half
//             wave read the same address: a broadcast), finds the equal bytes with zero8 and counts the five cases with __popcll into
//             32-bit registers kept for the whole span (a span has at most 2^30 columns).
//     fold    at the end of the span, not per tile, the lane adds the non-zero counters of its pairs to M[cls i][cls j] and
//             M[cls j][cls i] with 64-bit atomicAdd in device memory: integer sums, the same in any order of arrival.
//   host      argument checks before any launch (the walk over the groups and the checks of sbl_groups.h), the item list, the matrix cleared on the device before the launch and copied back after
//             it, both timed by event pairs.  SBL_TEST_GDIST_SPAN: test switch, the columns per span.
#include <algorithm>
#include <cstring>

#include "sbl_groups.h"

namespace {

constexpr unsigned GD_THREADS = 256;
constexpr unsigned GD_ROWS = 32;                       // rows of a row block
constexpr unsigned GD_TILE = 256;                      // columns of a tile
constexpr unsigned GD_WORDS = GD_TILE / 8 + 1;         // 64-bit words of an LDS row: the tile and 8 bytes of padding
constexpr unsigned GD_PAIRS = GD_ROWS * GD_ROWS / GD_THREADS;      // row pairs of a lane
constexpr u64 GD_TARGET = 2048;                        // items a call is cut into when its groups are few: 8 workgroups for each of 256 CUs
constexpr u64 GD_MIN_SPAN = 4096, GD_MAX_SPAN = 1ull << 30;      // columns of a span; the counters of a lane are 32 bit
constexpr u64 GD_HIGH = 0x8080808080808080ull, GD_GAPS = 0x2D2D2D2D2D2D2D2Dull;

struct GdItem { u64 toff, L, col0, col1, inst0; unsigned i0, ni, j0, nj; };      // rows [i0, i0 + ni) against [j0, j0 + nj), columns [col0, col1); inst0: the group's first instance

__global__ __launch_bounds__(GD_THREADS) void k_group_distances(const uint8_t *__restrict__ text, u64 text_bytes, const GdItem *__restrict__ items,
                                                                const unsigned *__restrict__ cls, unsigned nclass, unsigned long long *__restrict__ M)
{
	__shared__ u64 s_word[2][GD_ROWS][GD_WORDS], s_flag[2][GD_ROWS][GD_WORDS];
	const GdItem T = items[blockIdx.x];
	const bool diag = T.i0 == T.j0;
	const unsigned t = threadIdx.x, j = t % GD_ROWS, ib = t / GD_ROWS, side_j = diag ? 0 : 1;
	bool live[GD_PAIRS];
	unsigned n_match[GD_PAIRS], n_mis[GD_PAIRS], n_amb[GD_PAIRS], n_gij[GD_PAIRS], n_gji[GD_PAIRS];
	bool any = false;
#pragma unroll
	for (unsigned q = 0; q < GD_PAIRS; q++) {
		const unsigned i = ib + q * (GD_THREADS / GD_ROWS);
		live[q] = i < T.ni && j < T.nj && (!diag || i < j);
		any |= live[q];
		n_match[q] = n_mis[q] = n_amb[q] = n_gij[q] = n_gji[q] = 0;
	}
	const unsigned nrows = T.ni + (diag ? 0 : T.nj);
	for (u64 c0 = T.col0; c0 < T.col1; c0 += GD_TILE) {
		const unsigned w = T.col1 - c0 < GD_TILE ? (unsigned)(T.col1 - c0) : GD_TILE;      // columns of this tile
		const unsigned chunks = (w + 15) / 16;
		__syncthreads();                                                          // the sweep of the tile before is over
		for (unsigned x = t; x < nrows * chunks; x += GD_THREADS) {
			const unsigned r = x / chunks, k = x - r * chunks, side = r >= T.ni ? 1 : 0, lr = side ? r - T.ni : r;
			const u64 row = side ? T.j0 + lr : T.i0 + lr;
			B16 v = gv_load16(text, text_bytes, T.toff + row * T.L + c0 + 16 * k);
			if (w - 16 * k < 16) v = keep16(v, w - 16 * k, GD_GAPS);                      // behind the span: the next span, the next row or nothing
			s_word[side][lr][2 * k] = v.lo; s_word[side][lr][2 * k + 1] = v.hi;
			s_flag[side][lr][2 * k] = base_flags8(v.lo); s_flag[side][lr][2 * k + 1] = base_flags8(v.hi);
		}
		__syncthreads();
		if (!any) continue;
		for (unsigned k = 0; k < (w + 7) / 8; k++) {
			const u64 y = s_word[side_j][j][k], fy = s_flag[side_j][j][k], gy = (fy << 1) & GD_HIGH;
#pragma unroll
			for (unsigned q = 0; q < GD_PAIRS; q++) {
				if (!live[q]) continue;
				const unsigned i = ib + q * (GD_THREADS / GD_ROWS);
				const u64 x = s_word[0][i][k], fx = s_flag[0][i][k], gx = (fx << 1) & GD_HIGH;
				const u64 both = fx & fy & GD_HIGH, same = both & zero8(x ^ y);
				n_match[q] += __popcll(same);
				n_mis[q] += __popcll(both ^ same);
				n_amb[q] += __popcll(GD_HIGH & ~(gx | gy | both));
				n_gij[q] += __popcll(gy & ~gx);
				n_gji[q] += __popcll(gx & ~gy);
			}
		}
	}
#pragma unroll
	for (unsigned q = 0; q < GD_PAIRS; q++) {
		if (!live[q]) continue;
		const unsigned i = ib + q * (GD_THREADS / GD_ROWS);
		const u64 ci = cls[T.inst0 + T.i0 + i], cj = cls[T.inst0 + T.j0 + j];
		unsigned long long *const a = M + (ci * nclass + cj) * 4, *const b = M + (cj * nclass + ci) * 4;
		if (n_match[q]) { atomicAdd(a, (unsigned long long)n_match[q]); atomicAdd(b, (unsigned long long)n_match[q]); }
		if (n_mis[q]) { atomicAdd(a + 1, (unsigned long long)n_mis[q]); atomicAdd(b + 1, (unsigned long long)n_mis[q]); }
		if (n_amb[q]) { atomicAdd(a + 2, (unsigned long long)n_amb[q]); atomicAdd(b + 2, (unsigned long long)n_amb[q]); }
		if (n_gij[q]) atomicAdd(a + 3, (unsigned long long)n_gij[q]);
		if (n_gji[q]) atomicAdd(b + 3, (unsigned long long)n_gji[q]);
	}
}

}  // namespace

extern "C" sbl_status sbl_group_distances(sbl_ctx *c, const uint8_t *want, const uint32_t *cls, uint32_t nclass, const sbl_pair_counts **counts)
{
	return guarded(c, [&] {
		require_group_rows(c);
		const uint8_t *const rows = gm_reader_rows(c);
		check_classes(c, cls, nclass);
		const size_t ninst = c->gm_inst.size();
		hipStream_t s = c->stream;
		const size_t cells = (size_t)nclass * nclass;
		c->gd_counts.assign(cells, sbl_pair_counts{0, 0, 0, 0});
		c->gd_times = SblTimes{};
		// the wanted groups that have row pairs to compare, and the columns all their block pairs walk
		struct Wanted { size_t g; u64 nb; };
		std::vector<Wanted> groups;
		u64 work = 0;
		const GmListed listed = for_each_wanted_group(c, want, 2, [&](size_t g, const sbl_group_result &r, u64) {
			const u64 nb = (r.ninst + GD_ROWS - 1) / GD_ROWS;
			groups.push_back(Wanted{g, nb});
			work += nb * (nb + 1) / 2 * r.L;
		});
		if (!groups.empty()) {
			u64 span = std::max(GD_MIN_SPAN, (work / GD_TARGET + GD_TILE) / GD_TILE * GD_TILE);
			if (const char *e = getenv("SBL_TEST_GDIST_SPAN")) span = (u64)std::max(1ll, atoll(e));
			span = std::min(span, GD_MAX_SPAN);
			u64 nitems = 0;
			for (const Wanted &w : groups) nitems += w.nb * (w.nb + 1) / 2 * ((c->gm_res[w.g].L + span - 1) / span);      // at most the block pairs + GD_TARGET without the test switch
			SBL_CHECK(nitems < 0x7FFFFFFFull, SBL_ERR_TOO_LARGE, "alignment rows too large");
			std::vector<GdItem> items;
			items.reserve((size_t)nitems);
			for (const Wanted &w : groups) {
				const sbl_group_result &r = c->gm_res[w.g];
				for (u64 I = 0; I < w.nb; I++)
					for (u64 J = I; J < w.nb; J++)
						for (u64 col = 0; col < r.L; col += span)
							items.push_back(GdItem{r.row_off, r.L, col, std::min<u64>(r.L, col + span), c->gm_first[w.g], (unsigned)(I * GD_ROWS),
							                       (unsigned)std::min<u64>(GD_ROWS, r.ninst - I * GD_ROWS), (unsigned)(J * GD_ROWS),
							                       (unsigned)std::min<u64>(GD_ROWS, r.ninst - J * GD_ROWS)});
			}
			const u64 text_bytes = listed.text_bytes();
			require_rows_on_device(c, text_bytes, listed.n);
			al_upload(c, c->d_gd_item, items);
			c->d_gd_cls.ensure(ninst * sizeof(uint32_t));
			HIP_TRY(hipMemcpyAsync(c->d_gd_cls.p, cls, ninst * sizeof(uint32_t), hipMemcpyHostToDevice, s));
			c->d_gd_mat.ensure(cells * sizeof(sbl_pair_counts));
			HIP_TRY(hipEventRecord(c->ev[0], s));
			HIP_TRY(hipMemsetAsync(c->d_gd_mat.p, 0, cells * sizeof(sbl_pair_counts), s));
			k_group_distances<<<(unsigned)items.size(), GD_THREADS, 0, s>>>(rows, text_bytes, c->d_gd_item.as<GdItem>(), c->d_gd_cls.as<unsigned>(), nclass,
			                                                                c->d_gd_mat.as<unsigned long long>());
			HIP_TRY(hipGetLastError());
			HIP_TRY(hipEventRecord(c->ev[1], s));
			HIP_TRY(hipMemcpyAsync(c->gd_counts.data(), c->d_gd_mat.p, cells * sizeof(sbl_pair_counts), hipMemcpyDeviceToHost, s));
			HIP_TRY(hipEventRecord(c->ev[2], s));
			HIP_TRY(hipStreamSynchronize(s));
			c->gd_times.kernel_ms = sbl_elapsed_ms(c, 0, 1);
			c->gd_times.copy_ms = sbl_elapsed_ms(c, 1, 2);
			c->stats.device_bytes = sbl_devbuf_total().load();
		}
		if (counts) *counts = c->gd_counts.data();
	});
}

extern "C" sbl_status sbl_group_distances_times(const sbl_ctx *c, double *kernel_ms, double *copyback_ms)
{
	return sbl_times_out(c, &sbl_ctx::gd_times, kernel_ms, copyback_ms);
}
