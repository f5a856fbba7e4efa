// sbl_groups.h -- what the readers of the rows of the groups (group_variants.hip, group_distances.hip, group_concat.hip, group_boot.hip)
// share with each other and with k_spell_groups (block_align.hip), which spells those rows: the tables they are spelled from, the host's
// walk over the groups of the last groups call, its checks and tables; on the device the column walk, the tail cut, the centre bases
// before a column and the site flags of the two readers that take one row per class (k_site_flags).
#pragma once
#include <cstdio>

#include "sbl_align.h"
#include "sbl_text.h"

constexpr unsigned GM_THREADS = 256;                   // lanes of a workgroup of every kernel here and of the readers
constexpr unsigned GM_MAX_CLASS = 1024;                // classes a caller may give the instances

// the tables k_spell_groups spells the rows of the groups from; the readers find rows and centre indices through them
struct GmSlot { u64 col; unsigned p, G; };                                    // gap slot p: G columns from column col = p + the G of the slots before it
struct GmGroup { u64 toff, L, first_inst, first_slot; unsigned ninst, nslots; };      // toff: the group's text (ninst L bytes); slot 0 always listed
struct GmUsed { u64 group, dg; };                                             // a group a reader uses: its index in the call; its index in d_gm_group

// workgroups of GM_THREADS lanes for `lanes` lanes
inline unsigned gm_blocks(u64 lanes)
{
	const u64 blocks = (lanes + GM_THREADS - 1) / GM_THREADS;
	SBL_CHECK(blocks < 0x7FFFFFFFull, SBL_ERR_TOO_LARGE, "alignment rows too large");
	return (unsigned)blocks;
}

// what the readers ask for first: the rows of the last groups call are still on the device
inline void require_group_rows(const sbl_ctx *c)
{
	SBL_CHECK(c->gv_rows_valid, SBL_ERR_BAD_ARG, "no rows of groups on the device: the last sbl_align_* call must be sbl_align_groups or sbl_align_block_groups");
}
// the rows sbl_group_variants, sbl_group_distances and sbl_group_concat read, asked for before any launch: those of the groups call, or
// with sbl_group_set_masked on the masked rows of sbl_group_mask (group_mask.hip), a buffer of the same layout
inline const uint8_t *gm_reader_rows(const sbl_ctx *c)
{
	if (!c->gk_masked) return c->d_ga_text.as<uint8_t>();
	SBL_CHECK(c->gk_valid, SBL_ERR_BAD_ARG, "the masked rows are asked for (sbl_group_set_masked) and no sbl_group_mask call has made them since the last groups call");
	return c->d_gk_text.as<uint8_t>();
}
// ... and, once they know that they will launch: `listed` groups in d_gm_group, text_bytes of rows in d_ga_text
inline void require_rows_on_device(const sbl_ctx *c, u64 text_bytes, u64 listed)
{
	SBL_CHECK(c->d_ga_text.p && c->d_ga_text.cap >= text_bytes && c->d_gm_group.cap >= listed * sizeof(GmGroup), SBL_ERR_INTERNAL, "the rows of the groups are not on the device");
}

// the classes a caller gives the instances of the groups call
inline void check_classes(const sbl_ctx *c, const uint32_t *cls, uint32_t nclass)
{
	const size_t ninst = c->gm_inst.size();
	SBL_CHECK(cls || !ninst, SBL_ERR_BAD_ARG, "null classes");
	SBL_CHECK(nclass >= 1 && nclass <= GM_MAX_CLASS, SBL_ERR_BAD_ARG, "the number of classes must be 1 .. 1024");
	for (size_t k = 0; k < ninst; k++) SBL_CHECK(cls[k] < nclass, SBL_ERR_BAD_ARG, "a class is not below the number of classes");
}

// f(g, r, dg) for every wanted group g (want: null or one byte per group) that has min_rows rows at least, in ascending g; r: its result,
// dg: its place in d_gm_group, which lists the aligned groups with L > 0 in order.  Returns how many those are and where their rows end
// in d_ga_text
struct GmListed { u64 n, text_end; u64 text_bytes() const { return (text_end + 15) / 16 * 16; } };      // gv_load16 reads whole 16-byte words
template <class F> GmListed for_each_wanted_group(const sbl_ctx *c, const uint8_t *want, unsigned min_rows, F f)
{
	GmListed l{0, 0};
	for (size_t g = 0; g < c->gm_res.size(); g++) {
		const sbl_group_result &r = c->gm_res[g];
		if (r.status != SBL_GALIGN_OK || r.L == 0) continue;
		l.text_end = std::max<u64>(l.text_end, r.row_off + (u64)r.ninst * r.L);
		if (r.ninst >= min_rows && (!want || want[g])) f(g, r, l.n);
		l.n++;
	}
	return l;
}

// The groups of that walk as the column kernels take them: every group padded to a multiple of 16 columns, so that a lane's 16 columns
// lie in ONE group; cbase: the used.size() + 1 prefix of the padded columns.  f(g, r, dg) runs first for every group and may refuse it.
// Where there are groups, the rows are checked to be on the device and, with `upload`, the two tables go up into d_gm_used / d_gm_cbase
struct GmColumns { std::vector<GmUsed> used; std::vector<u64> cbase{0}; u64 text_bytes = 0; };
template <class F> GmColumns gm_columns(sbl_ctx *c, const uint8_t *want, unsigned min_rows, bool upload, F f)
{
	GmColumns t;
	const GmListed l = for_each_wanted_group(c, want, min_rows, [&](size_t g, const sbl_group_result &r, u64 dg) {
		f(g, r, dg);
		t.used.push_back(GmUsed{g, dg});
		t.cbase.push_back(t.cbase.back() + (r.L + 15) / 16 * 16);
	});
	t.text_bytes = l.text_bytes();
	if (!t.used.empty()) {
		require_rows_on_device(c, t.text_bytes, l.n);
		if (upload) { al_upload(c, c->d_gm_used, t.used); al_upload(c, c->d_gm_cbase, t.cbase); }
	}
	return t;
}

// The used groups of the readers that take one row per class (group_concat.hip, group_boot.hip): a used group holds every class exactly
// once, refused here before any launch.  roff[ug * nclass + f]: where the row of class f of used group ug starts in the rows; first: the
// nused + 1 prefix of the groups' columns.  One row is enough where there is one class.  Under sbl_group_set_partial (gp_partial, DESIGN.md
// 0.12) a used group holds every class AT MOST once: a group with fewer instances than classes is used, the roff of an absent class stays
// ~0 and the kernels' partial instantiations read it as "absent"; a class twice and more instances than classes are refused as before
[[noreturn]] inline void gm_bad_class_group(size_t g, const char *what)
{
	char b[160];
	snprintf(b, sizeof b, "group %zu %s: a used group holds every class exactly once", g, what);
	throw SblError{SBL_ERR_BAD_ARG, b};
}
inline GmColumns gm_class_columns(sbl_ctx *c, const uint8_t *want, const uint32_t *cls, uint32_t nclass, bool upload, std::vector<u64> &roff, std::vector<u64> &first)
{
	roff.clear(); first.assign(1, 0);
	return gm_columns(c, want, 1, upload, [&](size_t g, const sbl_group_result &r, u64) {
		if (r.ninst > nclass) gm_bad_class_group(g, "has more instances than there are classes");
		if (r.ninst < nclass && !c->gp_partial) gm_bad_class_group(g, "has fewer instances than there are classes");
		const size_t at = roff.size();
		roff.resize(at + nclass, ~0ull);
		for (u64 i = 0; i < r.ninst; i++) {
			u64 &slot = roff[at + cls[c->gm_first[g] + i]];
			if (slot != ~0ull) gm_bad_class_group(g, "holds a class twice");
			slot = r.row_off + i * r.L;
		}
		first.push_back(first.back() + r.L);
	});
}

// the first n bytes of w (0 < n < 16), `fill` (one byte, eight times) in every byte behind them
__device__ inline B16 keep16(B16 w, unsigned n, u64 fill)
{
	if (n < 8) { const u64 m = (1ull << (8 * n)) - 1; return {(w.lo & m) | (fill & ~m), fill}; }
	if (n == 8) return {w.lo, fill};
	const u64 m = (1ull << (8 * (n - 8))) - 1;
	return {w.lo, (w.hi & m) | (fill & ~m)};
}

// the merged gap slot of group Q that column col lies in or behind: the last one that starts at or before it (slot 0 starts at column 0)
__device__ inline u64 gm_slot_at(const GmSlot *__restrict__ slots, const GmGroup &Q, u64 col)
{
	return ga_find(0, Q.nslots, [&](u64 y) { return slots[Q.first_slot + y].col <= col; });
}
// column col is one of the gap columns of S, the slot gm_slot_at gives it
__device__ inline bool gm_in_slot(const GmSlot &S, u64 col) { return col - S.col < S.G; }
// the centre bases before column col = the centre index the column belongs to
__device__ inline u64 gm_centre_before(const GmSlot &S, u64 col) { return gm_in_slot(S, col) ? S.p : S.p + (col - S.col - S.G); }
__device__ inline u64 gm_centre_before(const GmSlot *__restrict__ slots, const GmGroup &Q, u64 col)
{
	return gm_centre_before(slots[Q.first_slot + gm_slot_at(slots, Q, col)], col);
}

// The column walk, output-stationary over the padded columns of the used groups: a lane owns 16 consecutive columns of ONE group, reads
// those 16 bytes of every row -- neighbouring lanes read neighbouring bytes of a row: 1 KiB per wave and row -- as two aligned 16-byte
// words shifted in registers (gv_load16: toff + i L is not aligned in general), compares them with row 0 8 bytes at a time and writes 16
// bytes with one vector store.  The reader R says what else it gathers and what the bytes are: rows(Q), the rows of group Q; first(ref)
// takes row 0 and next(w) every other row; bytes(ulo, uhi) gives the 16 bytes, ulo / uhi holding 0x80 in every byte whose column has a row
// that differs from row 0.  The bytes behind column L belong to the next row or to nothing: they are written as 0.
template <class R> __device__ inline void gm_walk16(const uint8_t *__restrict__ text, u64 text_bytes, const GmGroup *__restrict__ gm, const GmUsed *__restrict__ used,
                                                   const u64 *__restrict__ cbase, u64 nused, u64 padded_cols, R reader, uint4 *__restrict__ out)
{
	const u64 x0 = ((u64)blockIdx.x * GM_THREADS + threadIdx.x) * 16;
	if (x0 >= padded_cols) return;
	const unsigned gi = bs_find(cbase, nused, x0);
	const GmGroup Q = gm[used[gi].dg];
	const u64 col0 = x0 - cbase[gi];                                          // < L: the padding of a group is less than 16 columns
	const unsigned n = Q.L - col0 < 16 ? (unsigned)(Q.L - col0) : 16;        // columns of the group in this piece
	const unsigned rows = reader.rows(Q);
	const B16 ref = gv_load16(text, text_bytes, Q.toff + col0);
	reader.first(ref);
	u64 dlo = 0, dhi = 0;
	for (unsigned i = 1; i < rows; i++) {
		const B16 w = gv_load16(text, text_bytes, Q.toff + (u64)i * Q.L + col0);
		dlo |= w.lo ^ ref.lo; dhi |= w.hi ^ ref.hi;
		reader.next(w);
	}
	B16 o = reader.bytes(nonzero8(dlo), nonzero8(dhi));
	if (n < 16) o = keep16(o, n, 0);
	store16(out, x0 / 16, o);
}

// gm_walk16's reader of the site flags: bit 0 of a byte is set where the column holds one of A C G T in all of the group's rows and the
// rows are not all equal (SBL_CONCAT_VARIABLE's kept columns); with CLEAN, bit 1 where it holds one of A C G T in all rows, equal or not.
// PARTIAL (sbl_group_set_partial): the group's rows are the rows of the classes it holds, Q.ninst of them
template <bool CLEAN, bool PARTIAL = false> struct GcFlags {
	unsigned nclass;                                                          // a used group has nclass rows
	u64 alo, ahi;
	__device__ unsigned rows(const GmGroup &Q) const { return PARTIAL ? Q.ninst : nclass; }
	__device__ void first(B16 ref) { alo = base_flags8(ref.lo); ahi = base_flags8(ref.hi); }
	__device__ void next(B16 w) { alo &= base_flags8(w.lo); ahi &= base_flags8(w.hi); }
	__device__ B16 bytes(u64 ulo, u64 uhi) const
	{
		const u64 m = 0x8080808080808080ull;
		return {(ulo & alo) >> 7 | (CLEAN ? (alo & m) >> 6 : 0), (uhi & ahi) >> 7 | (CLEAN ? (ahi & m) >> 6 : 0)};
	}
};

template <bool CLEAN, bool PARTIAL = false>
__global__ __launch_bounds__(GM_THREADS) void k_site_flags(const uint8_t *__restrict__ text, u64 text_bytes, const GmGroup *__restrict__ gm,
                                                           const GmUsed *__restrict__ groups, const u64 *__restrict__ cbase, u64 ngroups,
                                                           u64 padded_cols, unsigned nclass, uint4 *__restrict__ flags)
{
	gm_walk16(text, text_bytes, gm, groups, cbase, ngroups, padded_cols, GcFlags<CLEAN, PARTIAL>{nclass, 0, 0}, flags);
}
