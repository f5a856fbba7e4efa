// group_boot.hip -- the bootstrap pair counts of the core-genome alignment (include/sibelia_amd.h): over the variable
// columns of the used groups of the last sbl_align_groups / sbl_align_block_groups call (the SITES: SBL_CONCAT_VARIABLE's kept columns),
// for every pair of CLASSES the caller gives the instances (the pipeline: the input file) the number of sites in which their rows
// differ -- once over all sites (slab 0) and once per bootstrap replicate, which draws sites with replacement by a counter-based rule.
// A replicate is the row comparisons of group_distances.hip once more on data that is already on the device, so they run there and only
// (replicates + 1) x nclass x nclass integers come back.
//
//   flags     k_site_flags<true> of sbl_groups.h: the column walk of group_concat.hip with a second flag bit, "every row holds one of
//             A C G T" whether the rows are equal or not.
//   clean     k_boot_clean counts that bit over the flag bytes (K): 16 bytes per lane, a wave sum by shuffles, one atomic per wave.
//   sites     the columns with bit 0 set are compacted in ascending order by rocPRIM's select (sbl_prim.h); the host reads C and K.
//   pack      k_boot_pack, one lane per (site, word): the SNP matrix in 2 bits per class, ceil(nclass / 32) 64-bit words per site, site
//             after site -- the 8-strain workload's 250 000 sites are 2 MB and stay in cache.  Every replicate draws from that.
//   count     k_boot_count, one launch for slab 0 and one per batch of replicates.  A workgroup owns GB_CHUNK draws of ONE replicate, a
//             block of GB_FB classes f and one word of 64 classes g; a wave takes 64 draws per step, a lane one of them: the draw rule in
//             registers, one load of the site's words, and per f the word XORed with f's base broadcast into every 2-bit field and folded
//             to one bit per class -- a 64-wide mask of "g differs from f" per lane.  The sum over the wave's 64 draws of bit g is the
//             popcount of the ballot of that bit, an exact integer, added into lane g's 32-bit register of f: no atomic and no LDS in the
//             loop.  A workgroup makes at most GB_CHUNK draws, so a register never passes GB_CHUNK whatever weight a site reaches (all
//             draws on one site included); at its end a lane adds its non-zero registers to M[r][f][g] and M[r][g][f] with 64-bit
//             atomicAdd in device memory: integer sums, the same in any order of arrival.  Only g > f is counted.
//   host      every argument is checked before any launch (the checks and the walk of sbl_groups.h); the slabs of a batch live in a device
//             buffer of at most GB_BUDGET bytes (SBL_TEST_BOOT_BUDGET_KB: test switch) and come back into the context's host array batch
//             after batch; one synchronise per batch, none per replicate.  SBL_TEST_BOOT_MAX_SITES: test switch, the limit on C.  Both
//             switches are for the tests only: read per call, a value below 1 or not a number counts as 1.  The packed sites stay in
//             d_gb_pack after the call, with their classes, their number and the partial setting recorded in the context
//             (gb_pack_valid): sbl_group_parsimony (group_parsimony.hip) reads them, no other call writes that buffer.
//   partial   under sbl_group_set_partial a used group holds every class at most once: the flags walk the rows the group
//             has, k_boot_clean_groups counts the clean columns per used group (the host folds them into the clean columns per pair of
//             classes, sbl_group_bootstrap_pairs), k_boot_pack<true> writes a presence word beside every base word and k_boot_count<true>
//             ANDs the difference mask with it.  The <false> instantiations are the kernels above, unchanged.
#include <algorithm>
#include <cstdlib>
#include <cstring>

#include "sbl_groups.h"
#include "sbl_prim.h"

namespace {

constexpr unsigned GB_THREADS = GM_THREADS, GB_WAVE = 64;
constexpr unsigned GB_FB = 8;                          // classes f of a workgroup: their registers
constexpr unsigned GB_CHUNK = 8192;                    // draws of a workgroup: 32 steps of each of its 4 waves
constexpr u64 GB_BUDGET = 64ull << 20;                 // bytes of count slabs on the device per batch of replicates
constexpr u64 GB_MAX_BLOCKS = 1ull << 22;              // workgroups of a launch in x (2^30 lanes)
constexpr u64 GB_MAX_CELLS = 1ull << 27;               // cells of the result: 1 GiB
constexpr u64 GB_LOW = 0x5555555555555555ull;

// flags: P bytes of k_site_flags<true>, 16 per lane; *K += the bytes with bit 1 set
__global__ __launch_bounds__(GB_THREADS) void k_boot_clean(const uint4 *__restrict__ flags, u64 words, unsigned long long *__restrict__ K)
{
	const u64 i = (u64)blockIdx.x * GB_THREADS + threadIdx.x;
	unsigned n = 0;
	if (i < words) {
		const uint4 v = flags[i];
		const unsigned m = 0x02020202u;
		n = __popc(v.x & m) + __popc(v.y & m) + __popc(v.z & m) + __popc(v.w & m);
	}
	for (unsigned d = GB_WAVE / 2; d; d >>= 1) n += __shfl_down(n, d, GB_WAVE);
	if (threadIdx.x % GB_WAVE == 0 && n) atomicAdd(K, (unsigned long long)n);
}

// PARTIAL's clean columns per used group: the same 16 bytes per lane, which lie in ONE group (its padded columns are a multiple of 16);
// K[gi] += the bytes with bit 1 set.  A wave that lies in one group sums by shuffles and adds once, a wave that straddles groups adds
// per lane.  Lanes of a wave ascend in i: where lane 0 is behind the flags, all are
__global__ __launch_bounds__(GB_THREADS) void k_boot_clean_groups(const uint4 *__restrict__ flags, u64 words, const u64 *__restrict__ cbase, u64 ngroups,
                                                                  unsigned long long *__restrict__ K)
{
	const u64 i = (u64)blockIdx.x * GB_THREADS + threadIdx.x;
	const bool live = i < words;
	unsigned n = 0, gi = 0;
	if (live) {
		const uint4 v = flags[i];
		const unsigned m = 0x02020202u;
		n = __popc(v.x & m) + __popc(v.y & m) + __popc(v.z & m) + __popc(v.w & m);
		gi = bs_find(cbase, ngroups, i * 16);
	}
	const unsigned g0 = __shfl(gi, 0, GB_WAVE);
	if (__all(!live || gi == g0)) {
		for (unsigned d = GB_WAVE / 2; d; d >>= 1) n += __shfl_down(n, d, GB_WAVE);
		if (threadIdx.x % GB_WAVE == 0 && n) atomicAdd(K + g0, (unsigned long long)n);
	} else if (n) atomicAdd(K + gi, (unsigned long long)n);
}

// packed[site * W + w]: the bases of classes 32 w .. 32 w + 31 in site `site`, class f in bits 2 (f % 32) and 2 (f % 32) + 1; a site
// holds one of A C G T in every row and (ch >> 1) & 3 tells them apart.  Classes behind nclass: 0.
// PARTIAL: a site is 2 W words, packed[site * 2 W + W + w] the presence of the same classes in the same layout -- bit 2 (f % 32) set where
// the site's group holds class f (roff != ~0); the base field of an absent class is 0
template <bool PARTIAL>
__global__ __launch_bounds__(GB_THREADS) void k_boot_pack(const uint8_t *__restrict__ text, const u64 *__restrict__ roff, const u64 *__restrict__ cbase, u64 ngroups,
                                                          const u64 *__restrict__ xs, u64 nsites, unsigned nclass, unsigned W, u64 *__restrict__ packed)
{
	const u64 i = (u64)blockIdx.x * GB_THREADS + threadIdx.x;
	if (i >= nsites * W) return;
	const u64 site = i / W;
	const unsigned w = (unsigned)(i - site * W);
	const u64 x = xs[site];
	const unsigned gi = bs_find(cbase, ngroups, x);
	const u64 col = x - cbase[gi];
	const unsigned f1 = nclass - 32 * w < 32 ? nclass - 32 * w : 32;
	u64 v = 0;
	if (PARTIAL) {
		u64 here = 0;
		for (unsigned k = 0; k < f1; k++) {
			const u64 r = roff[(u64)gi * nclass + 32 * w + k];
			if (r == ~0ull) continue;
			v |= (u64)((text[r + col] >> 1) & 3) << (2 * k);
			here |= 1ull << (2 * k);
		}
		packed[site * 2 * W + w] = v;
		packed[site * 2 * W + W + w] = here;
		return;
	}
	for (unsigned k = 0; k < f1; k++) v |= (u64)((text[roff[(u64)gi * nclass + 32 * w + k] + col] >> 1) & 3) << (2 * k);
	packed[i] = v;
}

// draw i of replicate r over C sites (include/sibelia_amd.h): splitmix64 of the counter, then a multiply-shift onto 0 .. C - 1
__device__ inline u64 gb_site(u64 seed, u64 r, u64 i, u64 C)
{
	u64 z = seed + 0x9E3779B97F4A7C15ull * (((r << 32) | i) + 1);
	z ^= z >> 30; z *= 0xBF58476D1CE4E5B9ull;
	z ^= z >> 27; z *= 0x94D049BB133111EBull;
	z ^= z >> 31;
	return ((z >> 32) * C) >> 32;
}

// blockIdx.x = (slab of the launch) * nchunks + chunk of its draws; blockIdx.y = (block of GB_FB classes f) * ngw + word of 64 classes g.
// slab0: the one slab is slab 0, whose draw i is site i (draws == C); otherwise slab l of the launch is replicate r0 + l.  M: the slabs of
// the launch, cleared by the host.  PARTIAL: a site is the 2 W words of k_boot_pack<true>; "g differs from f" counts only where the site's
// group holds g (an AND with the presence word of the g) and holds f (a select per f) -- ballots, popcounts and atomics as without
template <bool PARTIAL>
__global__ __launch_bounds__(GB_THREADS) void k_boot_count(const u64 *__restrict__ packed, unsigned W, u64 C, unsigned nclass, u64 seed, u64 r0, bool slab0,
                                                           u64 draws, unsigned nchunks, unsigned ngw, unsigned long long *__restrict__ M)
{
	const unsigned fb = blockIdx.y / ngw, gw = blockIdx.y - fb * ngw, f0 = fb * GB_FB;
	if (gw * 64 + 63 <= f0) return;                                           // no g > f in this word
	const u64 slab = blockIdx.x / nchunks, chunk = blockIdx.x - slab * nchunks;
	const unsigned lane = threadIdx.x % GB_WAVE;
	const u64 end = (chunk + 1) * GB_CHUNK < draws ? (chunk + 1) * GB_CHUNK : draws;
	const unsigned wf = f0 / 32, w0 = 2 * gw, w1 = 2 * gw + 1;                // the word that holds the block's f; the two words of the g
	const unsigned nf = nclass - f0 < GB_FB ? nclass - f0 : GB_FB;
	const unsigned g1 = nclass - gw * 64 < 64 ? nclass - gw * 64 : 64;       // classes of this word
	unsigned acc[GB_FB];
#pragma unroll
	for (unsigned k = 0; k < GB_FB; k++) acc[k] = 0;
	for (u64 i0 = chunk * GB_CHUNK + threadIdx.x / GB_WAVE * GB_WAVE; i0 < end; i0 += GB_THREADS) {      // uniform over the wave
		const u64 i = i0 + lane;
		const bool live = i < end;
		u64 xf = 0, x0 = 0, x1 = 0, pf = 0, p0 = 0, p1 = 0;
		if (live) {
			const u64 site = slab0 ? i : gb_site(seed, r0 + slab, i, C);
			const u64 *const p = packed + site * (PARTIAL ? 2 * W : W);
			xf = p[wf]; x0 = p[w0];
			if (w1 < W) x1 = p[w1];
			if (PARTIAL) {
				pf = p[W + wf]; p0 = p[W + w0];
				if (w1 < W) p1 = p[W + w1];
			}
		}
#pragma unroll
		for (unsigned k = 0; k < GB_FB; k++) {
			if (k >= nf) break;
			const unsigned f = f0 + k;
			const u64 bc = ((xf >> (2 * (f % 32))) & 3) * GB_LOW;
			const u64 y0 = x0 ^ bc, y1 = x1 ^ bc;
			u64 d0 = live ? (y0 | y0 >> 1) & GB_LOW : 0, d1 = live ? (y1 | y1 >> 1) & GB_LOW : 0;      // bit 2 j: class j of the word differs from f
			if (PARTIAL) {                                                        // ... and both are held; pf, p0, p1 are 0 in a lane that is not live
				const bool held = (pf >> (2 * (f % 32))) & 1;
				d0 = held ? d0 & p0 : 0; d1 = held ? d1 & p1 : 0;
			}
			const unsigned lo = f + 1 > gw * 64 ? f + 1 - gw * 64 : 0;       // the first g > f of this word
			unsigned add = 0;
			if (lo < 32) {
				d0 >>= 2 * lo;
				for (unsigned g = lo; g < (g1 < 32 ? g1 : 32); g++, d0 >>= 2) {
					const unsigned n = __popcll(__ballot(d0 & 1));
					if (lane == g) add = n;
				}
			}
			const unsigned hi = lo > 32 ? lo : 32;
			if (hi < g1) {
				d1 >>= 2 * (hi - 32);
				for (unsigned g = hi; g < g1; g++, d1 >>= 2) {
					const unsigned n = __popcll(__ballot(d1 & 1));
					if (lane == g) add = n;
				}
			}
			acc[k] += add;
		}
	}
	unsigned long long *const S = M + slab * nclass * nclass;
	const u64 g = (u64)gw * 64 + lane;
#pragma unroll
	for (unsigned k = 0; k < GB_FB; k++) {
		if (k >= nf || !acc[k]) continue;                                     // acc[k] != 0: lane is a g > f below nclass
		const u64 f = f0 + k;
		atomicAdd(S + f * nclass + g, (unsigned long long)acc[k]);
		atomicAdd(S + g * nclass + f, (unsigned long long)acc[k]);
	}
}

struct GbVariable { __host__ __device__ uint8_t operator()(uint8_t v) const { return v & 1; } };      // bit 0 of a flag byte: a site

u64 gb_env(const char *name, u64 scale, u64 dflt)
{
	const char *e = getenv(name);
	return e ? (u64)std::max(1ll, atoll(e)) * scale : dflt;
}

}  // namespace

extern "C" sbl_status sbl_group_bootstrap(sbl_ctx *c, const uint8_t *want, const uint32_t *cls, uint32_t nclass, uint32_t replicates, uint64_t seed, uint32_t draws,
                                          const uint64_t **counts, uint64_t *nsites, uint64_t *nclean)
{
	return guarded(c, [&] {
		require_group_rows(c);
		const uint8_t *const rows = gm_reader_rows(c);
		check_classes(c, cls, nclass);
		SBL_CHECK(replicates <= 100000, SBL_ERR_BAD_ARG, "the number of replicates must be 0 .. 100000");
		SBL_CHECK(counts, SBL_ERR_BAD_ARG, "null counts");
		const u64 cells = (u64)nclass * nclass, slabs = (u64)replicates + 1;
		SBL_CHECK(slabs * cells <= GB_MAX_CELLS, SBL_ERR_TOO_LARGE, "bootstrap counts too large: (replicates + 1) x classes x classes is limited to 2^27 cells");
		hipStream_t s = c->stream;
		c->gb_times = SblTimes{};
		std::vector<u64> roff, first;
		const GmColumns cols = gm_class_columns(c, want, cls, nclass, true, roff, first);
		const u64 ng = cols.used.size(), P = cols.cbase.back(), text_bytes = cols.text_bytes;
		const bool partial = c->gp_partial != 0;
		c->gb_counts.assign((size_t)(slabs * cells), 0);
		u64 CK[2] = {0, 0};                                                     // C, K
		std::vector<u64> gclean;                                                // partial: the clean columns of every used group
		if (ng) {
			// ---- the sites, ascending, their number and the number of clean columns
			c->d_gc_flag.ensure((size_t)P); c->d_gc_x.ensure((size_t)P * 8); c->d_gm_count.ensure(16);
			HIP_TRY(hipEventRecord(c->ev[0], s));
			HIP_TRY(hipMemsetAsync(c->d_gm_count.p, 0, 16, s));
			(partial ? k_site_flags<true, true> : k_site_flags<true, false>)<<<gm_blocks(P / 16), GB_THREADS, 0, s>>>(
				rows, text_bytes, c->d_gm_group.as<GmGroup>(), c->d_gm_used.as<GmUsed>(), c->d_gm_cbase.as<u64>(), ng, P, nclass, c->d_gc_flag.as<uint4>());
			HIP_TRY(hipGetLastError());
			if (partial) {
				c->d_gb_gclean.ensure((size_t)ng * 8);
				HIP_TRY(hipMemsetAsync(c->d_gb_gclean.p, 0, (size_t)ng * 8, s));
				k_boot_clean_groups<<<gm_blocks(P / 16), GB_THREADS, 0, s>>>(c->d_gc_flag.as<uint4>(), P / 16, c->d_gm_cbase.as<u64>(), ng, c->d_gb_gclean.as<unsigned long long>());
			} else
				k_boot_clean<<<gm_blocks(P / 16), GB_THREADS, 0, s>>>(c->d_gc_flag.as<uint4>(), P / 16, c->d_gm_count.as<unsigned long long>() + 1);
			HIP_TRY(hipGetLastError());
			const auto variable = rocprim::make_transform_iterator(c->d_gc_flag.as<uint8_t>(), GbVariable{});
			prim::select(s, c->d_gm_tmp, rocprim::counting_iterator<u64>(0), variable, c->d_gc_x.as<u64>(), c->d_gm_count.as<u64>(), (size_t)P);
			HIP_TRY(hipEventRecord(c->ev[1], s));
			HIP_TRY(hipMemcpyAsync(CK, c->d_gm_count.p, 16, hipMemcpyDeviceToHost, s));
			if (partial) {
				gclean.resize((size_t)ng);
				HIP_TRY(hipMemcpyAsync(gclean.data(), c->d_gb_gclean.p, (size_t)ng * 8, hipMemcpyDeviceToHost, s));
			}
			HIP_TRY(hipStreamSynchronize(s));
			c->gb_times.kernel_ms = sbl_elapsed_ms(c, 0, 1);
			for (const u64 k : gclean) CK[1] += k;
		}
		const u64 C = CK[0], n = draws ? draws : C;
		SBL_CHECK(C <= gb_env("SBL_TEST_BOOT_MAX_SITES", 1, 0xFFFFFFFFull), SBL_ERR_TOO_LARGE, "too many variable columns: the number of sites must be below 2^32");
		if (C) {
			const unsigned W = (nclass + 31) / 32, ngw = (nclass + 63) / 64, nfb = (nclass + GB_FB - 1) / GB_FB;
			const u64 nchunks0 = (C + GB_CHUNK - 1) / GB_CHUNK, nchunks = (n + GB_CHUNK - 1) / GB_CHUNK;      // both below 2^19
			// a batch: whole slabs within the budget (one at least) and within one launch's grid
			const u64 batch = std::max<u64>(1, std::min(gb_env("SBL_TEST_BOOT_BUDGET_KB", 1024, GB_BUDGET) / (cells * 8), GB_MAX_BLOCKS / nchunks));
			al_upload(c, c->d_gc_roff, roff);
			c->gb_pack_valid = false;                                            // the packed sites of the call before are written over from here on
			c->d_gb_pack.ensure((size_t)(C * W) * (partial ? 16 : 8));
			const auto pack = partial ? k_boot_pack<true> : k_boot_pack<false>;
			const auto count = partial ? k_boot_count<true> : k_boot_count<false>;
			c->d_gb_mat.ensure((size_t)(std::min<u64>(batch, slabs) * cells) * 8);
			unsigned long long *const M = c->d_gb_mat.as<unsigned long long>();
			// ---- the packed sites and slab 0
			HIP_TRY(hipEventRecord(c->ev[0], s));
			pack<<<gm_blocks(C * W), GB_THREADS, 0, s>>>(rows, c->d_gc_roff.as<u64>(), c->d_gm_cbase.as<u64>(), ng, c->d_gc_x.as<u64>(), C, nclass, W, c->d_gb_pack.as<u64>());
			HIP_TRY(hipGetLastError());
			HIP_TRY(hipMemsetAsync(M, 0, (size_t)cells * 8, s));
			count<<<dim3((unsigned)nchunks0, nfb * ngw), GB_THREADS, 0, s>>>(c->d_gb_pack.as<u64>(), W, C, nclass, seed, 0, true, C, (unsigned)nchunks0, ngw, M);
			HIP_TRY(hipGetLastError());
			HIP_TRY(hipEventRecord(c->ev[1], s));
			HIP_TRY(hipMemcpyAsync(c->gb_counts.data(), M, (size_t)cells * 8, hipMemcpyDeviceToHost, s));
			HIP_TRY(hipEventRecord(c->ev[2], s));
			HIP_TRY(hipStreamSynchronize(s));
			c->gb_times.kernel_ms += sbl_elapsed_ms(c, 0, 1);
			c->gb_times.copy_ms += sbl_elapsed_ms(c, 1, 2);
			// ---- the replicates, batch after batch
			for (u64 r = 1; r <= replicates; r += batch) {
				const u64 nb = std::min<u64>(batch, replicates - r + 1);
				HIP_TRY(hipEventRecord(c->ev[0], s));
				HIP_TRY(hipMemsetAsync(M, 0, (size_t)(nb * cells) * 8, s));
				count<<<dim3((unsigned)(nb * nchunks), nfb * ngw), GB_THREADS, 0, s>>>(c->d_gb_pack.as<u64>(), W, C, nclass, seed, r, false, n, (unsigned)nchunks, ngw, M);
				HIP_TRY(hipGetLastError());
				HIP_TRY(hipEventRecord(c->ev[1], s));
				HIP_TRY(hipMemcpyAsync(c->gb_counts.data() + r * cells, M, (size_t)(nb * cells) * 8, hipMemcpyDeviceToHost, s));
				HIP_TRY(hipEventRecord(c->ev[2], s));
				HIP_TRY(hipStreamSynchronize(s));
				c->gb_times.kernel_ms += sbl_elapsed_ms(c, 0, 1);
				c->gb_times.copy_ms += sbl_elapsed_ms(c, 1, 2);
			}
		}
		// ---- the clean columns per pair of classes: those of the groups that hold both, through the presence roff carries
		c->gb_pairs.assign((size_t)cells, partial ? 0 : CK[1]);
		if (partial) {
			std::vector<uint32_t> held;
			for (u64 u = 0; u < ng; u++) {
				if (!gclean[u]) continue;
				held.clear();
				for (uint32_t f = 0; f < nclass; f++) if (roff[u * nclass + f] != ~0ull) held.push_back(f);
				for (const uint32_t f : held) for (const uint32_t g : held) c->gb_pairs[(size_t)f * nclass + g] += gclean[u];
			}
		}
		c->gb_pairs_valid = true;
		c->gb_pack_valid = true;                                                // d_gb_pack holds the C sites of this call: what sbl_group_parsimony reads
		c->gb_pack_nclass = nclass; c->gb_pack_partial = partial; c->gb_pack_sites = C;
		c->stats.device_bytes = sbl_devbuf_total().load();
		*counts = c->gb_counts.data();
		if (nsites) *nsites = C;
		if (nclean) *nclean = CK[1];
	});
}

extern "C" sbl_status sbl_group_bootstrap_pairs(sbl_ctx *c, const uint64_t **clean)
{
	return guarded(c, [&] {
		SBL_CHECK(clean, SBL_ERR_BAD_ARG, "null clean");
		SBL_CHECK(c->gb_pairs_valid, SBL_ERR_BAD_ARG, "no clean columns per pair: no sbl_group_bootstrap call has succeeded yet");
		*clean = c->gb_pairs.data();
	});
}

extern "C" sbl_status sbl_group_bootstrap_times(const sbl_ctx *c, double *kernel_ms, double *copyback_ms)
{
	return sbl_times_out(c, &sbl_ctx::gb_times, kernel_ms, copyback_ms);
}
