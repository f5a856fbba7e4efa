// uncovered.hip -- what the reference's comparison tool C-Sibelia.py calls from the regions no block covers (src/csibelia/C-Sibelia.py
// :325-338 depict_coverage, :373-427 the walk over the uncovered runs).
//
//   sbl_uncovered_calls   HOST.  C-Sibelia paints one array cell per base; here the same result comes from intervals: per list the ids
//           with an instance on and an instance off the reference records (mixed), the union of their instances per record by one sort,
//           the complement runs longer than min_block_size, and for a run of an assembly record the mixed instance of the FINAL list that
//           holds the base before it (the largest id: C-Sibelia's last writer) with the rule that anchors the insertion.  The host is the
//           right place: the number of runs follows the number of block instances, not of bases, the block lists are host arrays already
//           and nothing here touches a base -- the division DESIGN.md 0.3 argues for the merge of the gap slots.
//   The text of the calls (REF / ALT of a VCF line, the FASTA of the unmapped insertions) is spelled on the device: sbl_spell_text,
//   spell_text.hip.
#include <algorithm>
#include <cstring>

#include "sbl_align.h"

namespace {

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
