// sbl_align.h -- what boundary_align.hip and block_align.hip share: the scores, the read of a base on its strand, the timed launch, the
// argument checks, the walk over the instances of one block and the group tables of the row speller.
#pragma once
#include <algorithm>
#include <cstdlib>

#include "sbl_ctx.h"
#include "sbl_dna.h"

typedef unsigned long long u64;

constexpr int AL_MATCH = 25, AL_PENALTY = 75;          // match; mismatch and gap column (32 bit)

// base i of the len bases at seq + src as its strand spells them: a reverse range is read downwards through complement1
__device__ inline unsigned char strand_base(const uint8_t *__restrict__ seq, u64 src, unsigned len, unsigned i, bool rev)
{
	return rev ? complement1(seq[src + (len - 1 - i)]) : seq[src + i];
}

template <class F> __device__ inline u64 ga_find(u64 lo, u64 hi, F le)   // largest x in [lo, hi) with le(x) (le(lo) holds)
{
	while (hi - lo > 1) {
		const u64 mid = lo + (hi - lo) / 2;
		if (le(mid)) lo = mid; else hi = mid;
	}
	return lo;
}

// the tables k_spell_groups spells the rows of the groups from (block_align.hip); group_variants.hip reads the rows through them
struct GmSlot { u64 col; unsigned p, G; };                                    // gap slot p: G columns from column col = p + the G of the slots before it
struct GmGroup { u64 toff, L, first_inst, first_slot; unsigned ninst, nslots; };      // toff: the group's text (ninst L bytes); slot 0 always listed

// `launch` between ev[0] and ev[1], `bytes` of its results back to the host and one synchronise -> the milliseconds between the events
template <class F> float al_timed_launch(sbl_ctx *c, F launch, void *back, const void *d_from, size_t bytes)
{
	hipStream_t s = c->stream;
	HIP_TRY(hipEventRecord(c->ev[0], s));
	launch();
	HIP_TRY(hipGetLastError());
	HIP_TRY(hipEventRecord(c->ev[1], s));
	HIP_TRY(hipMemcpyAsync(back, d_from, bytes, hipMemcpyDeviceToHost, s));
	HIP_TRY(hipStreamSynchronize(s));
	return sbl_elapsed_ms(c, 0, 1);
}

// a table of descriptors into its device buffer, grown to hold it
template <class T> void al_upload(sbl_ctx *c, DevBuf &d, const std::vector<T> &v)
{
	d.ensure(std::max<size_t>(1, v.size()) * sizeof(T));
	if (!v.empty()) HIP_TRY(hipMemcpyAsync(d.p, v.data(), v.size() * sizeof(T), hipMemcpyHostToDevice, c->stream));
}

inline void require_reference_split(const sbl_ctx *c, uint32_t n_reference_chr)
{
	SBL_CHECK(n_reference_chr > 0 && n_reference_chr < c->nchr, SBL_ERR_BAD_ARG, "the reference set must hold at least one record and leave at least one outside it");
}

// one range of a record; no_record: the caller's words for a record that does not exist
inline void check_range(const sbl_ctx *c, uint32_t chr, uint64_t start, uint64_t end, const char *no_record)
{
	SBL_CHECK(chr < c->nchr, SBL_ERR_BAD_ARG, no_record);
	SBL_CHECK(end >= start, SBL_ERR_BAD_ARG, "a range ends before it starts");
	SBL_CHECK(end <= (uint64_t)(c->orig_sepidx[chr + 1] - c->orig_sepidx[chr] - 1), SBL_ERR_BAD_ARG, "a range runs beyond its record");
}

// what sbl_group_variants and sbl_group_distances ask for first: the rows of the last groups call are still on the device
inline void require_group_rows(const sbl_ctx *c)
{
	SBL_CHECK(c->gv_rows_valid, SBL_ERR_BAD_ARG, "no rows of groups on the device: the last sbl_align_* call must be sbl_align_groups or sbl_align_block_groups");
}

// f(g, r, dg) for every wanted group g (want: null or one byte per group) that has rows to compare with each other; r: its result, dg: its
// place in d_gm_group, which lists the aligned groups with L > 0 in order.  Returns how many those are and where their rows end in d_ga_text
struct GmListed { u64 n, text_end; };
template <class F> GmListed for_each_wanted_group(const sbl_ctx *c, const uint8_t *want, F f)
{
	GmListed l{0, 0};
	for (size_t g = 0; g < c->gm_res.size(); g++) {
		const sbl_group_result &r = c->gm_res[g];
		if (r.status != SBL_GALIGN_OK || r.L == 0) continue;
		l.text_end = std::max<u64>(l.text_end, r.row_off + (u64)r.ninst * r.L);
		if (r.ninst >= 2 && (!want || want[g])) f(g, r, l.n);
		l.n++;
	}
	return l;
}

// f(i, j) for every run v[i .. j) of equal |id| of a list sorted by |id|; f may change the run it is given
template <class F> void for_each_id_run(const std::vector<sbl_block> &v, F f)
{
	for (size_t i = 0, j; i < v.size(); i = j) {
		const int id = std::abs(v[i].id);
		for (j = i + 1; j < v.size() && std::abs(v[j].id) == id; j++) {}
		f(i, j);
	}
}
