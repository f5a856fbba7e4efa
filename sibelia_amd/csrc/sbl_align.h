// sbl_align.h -- what boundary_align.hip and block_align.hip share: the scores, the read of a base on its strand, the timed launch, the
// argument checks and the walk over the instances of one block.  What the rows of the groups need is in sbl_groups.h.
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

// f(i, j) for every run v[i .. j) of equal |id| of a list sorted by |id|; f may change the run it is given
template <class F> void for_each_id_run(const std::vector<sbl_block> &v, F f)
{
	for (size_t i = 0, j; i < v.size(); i = j) {
		const int id = std::abs(v[i].id);
		for (j = i + 1; j < v.size() && std::abs(v[j].id) == id; j++) {}
		f(i, j);
	}
}
