// blockseq.hip -- OutputGenerator::ListBlocksSequences (reference src/outputgenerator.cpp:287-318 with OutputLines :102-113): the text of
// blocks_sequences.fasta, spelled on the device from the ORIGINAL records by k_spell_text (spell_text.hip).  Here is the front end:
// the reference's order (one unstable std::sort by |id| of a copy of the list: the same libstdc++ call on the same element order,
// postprocess.hip's group_by / ById), the header lines as one blob, and per instance two pieces -- the header as a literal range of the
// blob, and the bases as a record range in lines of 80, read downwards through the complement for id < 0, case kept.  An instance
// without bases has no second piece (a wrapped empty range spells nothing): its line feed is one more byte of its literal.
#include <algorithm>
#include <cstring>

#include "sbl_ctx.h"
#include "sbl_text.h"

// checks shared by the two reports that take a caller's list
void sbl_check_blocks(const sbl_ctx *c, const sbl_block *b, uint64_t n)
{
	require_records(c);
	SBL_CHECK(n == 0 || b, SBL_ERR_BAD_ARG, "null block list");
	for (uint64_t i = 0; i < n; i++) {
		SBL_CHECK(b[i].id != 0, SBL_ERR_BAD_ARG, "block id 0");
		SBL_CHECK(b[i].chr < c->nchr, SBL_ERR_BAD_ARG, "block instance on a record that does not exist");
		SBL_CHECK(b[i].end >= b[i].start, SBL_ERR_BAD_ARG, "block instance ends before it starts");
		SBL_CHECK(b[i].end <= (uint64_t)(c->orig_sepidx[b[i].chr + 1] - c->orig_sepidx[b[i].chr] - 1), SBL_ERR_BAD_ARG, "block instance runs beyond its record");
	}
}

extern "C" sbl_status sbl_blocks_sequences(sbl_ctx *c, const sbl_block *blocks, uint64_t n, const char *const *names, const char **text, uint64_t *len)
{
	return guarded(c, [&] {
		if (!blocks) { blocks = c->blocks.data(); n = c->blocks.size(); }
		sbl_check_blocks(c, blocks, n);
		std::vector<sbl_block> v(blocks, blocks + n);
		sbl_sort_by_id(v);
		// header blob, pieces, offsets
		std::string hdr;
		std::vector<StDesc> desc;
		std::vector<u64> toff(1, 0);
		desc.reserve(2 * n); toff.reserve(2 * n + 1);
		char num[96];
		for (uint64_t i = 0; i < n; i++) {
			const sbl_block &b = v[i];
			const bool fwd = b.id > 0;
			const u64 from = fwd ? b.start + 1 : b.end, to = fwd ? b.end : b.start + 1, L = b.end - b.start;      // src/blockinstance.cpp:57-75
			const u64 hoff = hdr.size();
			hdr += ">Seq=\"";
			hdr += names ? names[b.chr] : b.chr < c->fa_names.size() ? c->fa_names[b.chr].c_str() : "";
			snprintf(num, sizeof num, "\",Strand='%c',Block_id=%d,Start=%llu,End=%llu\n", fwd ? '+' : '-', b.id > 0 ? b.id : -b.id, from, to);
			hdr += num;
			SBL_CHECK(hdr.size() - hoff < 0xFFFFFFFFull, SBL_ERR_TOO_LARGE, "record description too long");
			if (!L) hdr += '\n';
			desc.push_back(StDesc{hoff, hdr.size() - hoff, 0, ST_LITERAL});
			toff.push_back(toff.back() + desc.back().L);
			if (!L) continue;
			desc.push_back(StDesc{(u64)c->orig_sepidx[b.chr] + 1 + b.start, L, 80, ST_KEEP_CASE | (fwd ? 0 : ST_REVERSE)});
			toff.push_back(toff.back() + st_text_len(L, 80));
		}
		sbl_spell_pieces(c, desc, toff, hdr.data(), hdr.size(), "blocks_sequences text too large", c->bs_times);
		if (text) *text = toff.back() ? c->h_bs_text.p : "";
		if (len) *len = toff.back();
	});
}

extern "C" sbl_status sbl_blocks_sequences_times(const sbl_ctx *c, double *kernel_ms, double *copyback_ms)
{
	return sbl_times_out(c, &sbl_ctx::bs_times, kernel_ms, copyback_ms);
}
