// group_parsimony.hip -- Fitch parsimony of the sites of the core-genome alignment on a tree (include/sibelia_amd.h): per
// site its steps and the least a site with its bases can take, per change the site, the edge and the two bases, per edge the changes by
// kind.  The sites are the packed words the last sbl_group_bootstrap call left on the device (group_boot.hip: k_boot_pack), the tree
// comes from the caller as sbl_nj_batch hands it out.  Everything is integers.
//
//   schedule  the host reads the tree from leaf 0 and turns it into one table of 32-bit words, the same for every lane: per internal node
//             in postorder (top last) the node and its two children, then per edge of the caller the node below it and the node above.
//             A kernel reads it through uniform indices only.
//   sets      a lane owns one site.  The sets of all 2 n - 2 nodes live in LDS as bytes [node][lane]: a lane reads and writes its own
//             column only, so no barrier orders them.  The site's words (W = ceil(n / 32), 2 W with presence) are loaded once into named
//             registers; the leaf loop is uniform.
//   steps     k_fitch_steps: the leaf sets, bottom-up over the schedule, the test at the top; steps and minsteps, one byte each.
//   scan      rocPRIM's exclusive scan (sbl_prim.h) of the steps to 64-bit offsets over C + 1 bytes, the last one 0: offset C is the
//             total, which the host reads.
//   changes   k_fitch_changes: bottom-up again, then top-down in the reverse schedule, a node's state written over its set; then the
//             caller's edges in ascending index: where the two states differ one record at the site's offset (never at or behind the
//             total) and one add into the workgroup's LDS histogram [edge][16], whose non-zero cells go to the counts with 64-bit
//             atomicAdd -- integer sums, the same in any order.
//   host      every argument is checked before any launch; results are made in fresh arrays and take the place of the context's only
//             where the call succeeds.  SBL_TEST_PARSIMONY_MAX_CHANGES: test switch, the limit on the change list.
#include <algorithm>
#include <cstdlib>
#include <cstring>

#include "sbl_groups.h"
#include "sbl_prim.h"

namespace {

constexpr unsigned GF_THREADS = 256;
constexpr unsigned GF_MAX = 64;                        // leaves: sbl_nj_batch's limit
constexpr u64 GF_MAX_CHANGES = 1ull << 26;             // records of 16 bytes: 1 GiB

struct GfByte { __host__ __device__ u64 operator()(uint8_t v) const { return v; } };

// the leaf sets of `site` into the lane's column of S; -> the union of the sets of the present leaves
template <bool PARTIAL>
__device__ inline unsigned gf_leaves(const u64 *__restrict__ packed, unsigned W, u64 site, unsigned n, uint8_t *S)
{
	const u64 *const p = packed + site * (PARTIAL ? 2 * W : W);
	const u64 b0 = p[0], b1 = W > 1 ? p[1] : 0;
	u64 h0 = 0, h1 = 0;
	if (PARTIAL) { h0 = p[W]; h1 = W > 1 ? p[W + 1] : 0; }
	unsigned seen = 0;
	for (unsigned f = 0; f < n; f++) {                                         // uniform
		const unsigned sh = 2 * (f % 32);
		const unsigned set = 1u << ((unsigned)((f < 32 ? b0 : b1) >> sh) & 3);
		if (PARTIAL && !(((f < 32 ? h0 : h1) >> sh) & 1)) { S[f * GF_THREADS] = 0xF; continue; }
		S[f * GF_THREADS] = (uint8_t)set;
		seen |= set;
	}
	return seen;
}

// bottom-up over the schedule and the test at the top -> the steps of the site
__device__ inline unsigned gf_up(const uint32_t *__restrict__ sched, unsigned n, uint8_t *S)
{
	unsigned steps = 0;
	for (unsigned k = 0; k + 2 < n; k++) {                                     // uniform
		const uint32_t e = sched[k];
		const unsigned a = S[((e >> 8) & 0xFF) * GF_THREADS], b = S[((e >> 16) & 0xFF) * GF_THREADS];
		unsigned x = a & b;
		if (!x) { x = a | b; steps++; }
		S[(e & 0xFF) * GF_THREADS] = (uint8_t)x;
	}
	const unsigned top = sched[n - 3] & 0xFF;
	if (!(S[0] & S[top * GF_THREADS])) steps++;
	return steps;
}

template <bool PARTIAL>
__global__ __launch_bounds__(GF_THREADS) void k_fitch_steps(const u64 *__restrict__ packed, unsigned W, u64 C, unsigned n, const uint32_t *__restrict__ sched,
                                                            uint8_t *__restrict__ steps, uint8_t *__restrict__ minsteps)
{
	extern __shared__ uint8_t gf_lds[];                                        // (2 n - 2) * GF_THREADS bytes
	const u64 site = (u64)blockIdx.x * GF_THREADS + threadIdx.x;
	if (site >= C) return;
	uint8_t *const S = gf_lds + threadIdx.x;
	const unsigned seen = gf_leaves<PARTIAL>(packed, W, site, n, S);
	steps[site] = (uint8_t)gf_up(sched, n, S);
	minsteps[site] = (uint8_t)(seen ? __popc(seen) - 1 : 0);
}

// off: the C + 1 offsets of the scan, total = off[C]; counts: (2 n - 3) * 16 cells, cleared by the host
template <bool PARTIAL>
__global__ __launch_bounds__(GF_THREADS) void k_fitch_changes(const u64 *__restrict__ packed, unsigned W, u64 C, unsigned n, const uint32_t *__restrict__ sched,
                                                              const u64 *__restrict__ off, u64 total, ulonglong2 *__restrict__ changes,
                                                              unsigned long long *__restrict__ counts)
{
	extern __shared__ uint8_t gf_lds[];                                        // the sets, then the histogram
	const unsigned ne = 2 * n - 3;
	unsigned *const H = reinterpret_cast<unsigned *>(gf_lds + (2 * n - 2) * GF_THREADS);
	for (unsigned i = threadIdx.x; i < ne * 16; i += GF_THREADS) H[i] = 0;
	__syncthreads();
	const u64 site = (u64)blockIdx.x * GF_THREADS + threadIdx.x;
	if (site < C) {
		uint8_t *const S = gf_lds + threadIdx.x;
		gf_leaves<PARTIAL>(packed, W, site, n, S);
		gf_up(sched, n, S);
		// top-down: a state takes the place of its node's set once the set is read
		const unsigned top = sched[n - 3] & 0xFF;
		const unsigned s0 = S[0] == 0xF ? __ffs((unsigned)S[top * GF_THREADS]) - 1 : __ffs((unsigned)S[0]) - 1;
		S[0] = (uint8_t)s0;
		{
			const unsigned set = S[top * GF_THREADS];
			S[top * GF_THREADS] = (uint8_t)((set >> s0) & 1 ? s0 : __ffs(set) - 1);
		}
		for (unsigned k = n - 2; k-- > 0;) {                                   // uniform
			const uint32_t e = sched[k];
			const unsigned pv = S[(e & 0xFF) * GF_THREADS];
			const unsigned ia = ((e >> 8) & 0xFF) * GF_THREADS, ib = ((e >> 16) & 0xFF) * GF_THREADS;
			const unsigned sa = S[ia], sb = S[ib];
			S[ia] = (uint8_t)((sa >> pv) & 1 ? pv : __ffs(sa) - 1);
			S[ib] = (uint8_t)((sb >> pv) & 1 ? pv : __ffs(sb) - 1);
		}
		u64 at = off[site];
		for (unsigned e = 0; e < ne; e++) {                                    // uniform
			const uint32_t w = sched[n - 2 + e];
			const unsigned to = S[(w & 0xFF) * GF_THREADS], from = S[((w >> 8) & 0xFF) * GF_THREADS];
			if (to == from) continue;
			if (at < total) changes[at] = make_ulonglong2(site, (u64)e | (u64)from << 32 | (u64)to << 40);
			at++;
			atomicAdd(H + e * 16 + from * 4 + to, 1u);
		}
	}
	__syncthreads();
	for (unsigned i = threadIdx.x; i < ne * 16; i += GF_THREADS)
		if (H[i]) atomicAdd(counts + i, (unsigned long long)H[i]);
}

// the tree read from leaf 0 -> the schedule; refuses what is not a binary tree over leaves 0 .. n - 1 and internal nodes n .. 2 n - 3
std::vector<uint32_t> gf_schedule(const sbl_nj_edge *edges, unsigned n)
{
	const unsigned nn = 2 * n - 2, ne = 2 * n - 3;
	std::vector<std::vector<std::pair<unsigned, unsigned>>> adj(nn);          // (neighbour, edge)
	for (unsigned e = 0; e < ne; e++) {
		const unsigned u = edges[e].parent, v = edges[e].child;
		SBL_CHECK(u < nn && v < nn, SBL_ERR_BAD_ARG, "an edge names a node that is not below 2 n - 2");
		adj[u].push_back({v, e});
		adj[v].push_back({u, e});
	}
	for (unsigned v = 0; v < nn; v++)
		SBL_CHECK(adj[v].size() == (v < n ? 1u : 3u), SBL_ERR_BAD_ARG, "the edges are not a binary tree: every leaf has one edge and every internal node three");
	const unsigned top = adj[0][0].first;
	SBL_CHECK(top >= n, SBL_ERR_BAD_ARG, "the edges are not a tree: leaf 0 hangs on a leaf");
	// preorder from top; 2 n - 3 edges join 2 n - 2 nodes: a tree iff every node is reached
	std::vector<unsigned> parent(nn, ~0u), pedge(nn, 0), order, stack{top};
	std::vector<bool> seen(nn, false);
	parent[top] = 0; pedge[top] = adj[0][0].second;
	seen[0] = seen[top] = true;
	while (!stack.empty()) {
		const unsigned v = stack.back();
		stack.pop_back();
		order.push_back(v);
		for (const auto &[w, e] : adj[v]) {
			if (e == pedge[v]) continue;
			SBL_CHECK(!seen[w], SBL_ERR_BAD_ARG, "the edges are not a tree: they close a cycle");
			seen[w] = true; parent[w] = v; pedge[w] = e;
			stack.push_back(w);
		}
	}
	SBL_CHECK(order.size() == nn - 1, SBL_ERR_BAD_ARG, "the edges are not a tree: not every node hangs together with leaf 0");
	std::vector<uint32_t> sched(n - 2 + ne);
	unsigned k = n - 2;
	for (const unsigned v : order) {                                           // the reverse of a preorder: children before their parent, top last
		if (v < n) continue;
		unsigned kid[2], nk = 0;
		for (const auto &[w, e] : adj[v]) if (e != pedge[v]) kid[nk++] = w;
		sched[--k] = v | kid[0] << 8 | kid[1] << 16;
	}
	for (unsigned v = 1; v < nn; v++) sched[n - 2 + pedge[v]] = v | parent[v] << 8;
	return sched;
}

u64 gf_env(const char *name, u64 dflt)
{
	const char *e = getenv(name);
	return e ? (u64)std::max(1ll, atoll(e)) : dflt;
}

}  // namespace

static_assert(sizeof(sbl_parsimony_change) == 16 && sizeof(ulonglong2) == 16, "a change record is one 16-byte store");

extern "C" sbl_status sbl_group_parsimony(sbl_ctx *c, const sbl_nj_edge *edges, uint32_t n, const uint64_t **edge_counts, const uint8_t **steps, const uint8_t **minsteps,
                                          const sbl_parsimony_change **changes, uint64_t *nchanges)
{
	return guarded(c, [&] {
		SBL_CHECK(edge_counts && steps && minsteps && changes && nchanges, SBL_ERR_BAD_ARG, "null result pointer");
		SBL_CHECK(edges, SBL_ERR_BAD_ARG, "null edges");
		SBL_CHECK(c->gb_pack_valid, SBL_ERR_BAD_ARG, "no sites: no sbl_group_bootstrap call has succeeded yet");
		SBL_CHECK(n >= 3, SBL_ERR_BAD_ARG, "a tree takes three or more leaves");
		SBL_CHECK(n <= GF_MAX, SBL_ERR_TOO_LARGE, "parsimony on the device takes at most 64 leaves");
		SBL_CHECK(n == c->gb_pack_nclass, SBL_ERR_BAD_ARG, "the number of leaves is not the number of classes of the last sbl_group_bootstrap call");
		const std::vector<uint32_t> sched = gf_schedule(edges, n);
		const u64 C = c->gb_pack_sites, ne = 2 * (u64)n - 3;
		const bool partial = c->gb_pack_partial != 0;
		std::vector<uint64_t> counts((size_t)ne * 16, 0);
		std::vector<uint8_t> st((size_t)C), mn((size_t)C);
		std::vector<sbl_parsimony_change> ch;
		SblTimes times{};
		if (C) {
			hipStream_t s = c->stream;
			const unsigned W = (n + 31) / 32, blocks = (unsigned)((C + GF_THREADS - 1) / GF_THREADS);      // C < 2^32
			const size_t lds_sets = (size_t)(2 * n - 2) * GF_THREADS, lds_all = lds_sets + (size_t)ne * 16 * 4;
			c->d_gf_sched.ensure(sched.size() * 4);
			c->d_gf_steps.ensure((size_t)C + 1); c->d_gf_min.ensure((size_t)C); c->d_gf_off.ensure((size_t)(C + 1) * 8); c->d_gf_counts.ensure((size_t)ne * 16 * 8);
			HIP_TRY(hipMemcpyAsync(c->d_gf_sched.p, sched.data(), sched.size() * 4, hipMemcpyHostToDevice, s));
			u64 total = 0;
			HIP_TRY(hipEventRecord(c->ev[0], s));
			HIP_TRY(hipMemsetAsync(c->d_gf_steps.as<uint8_t>() + C, 0, 1, s));
			(partial ? k_fitch_steps<true> : k_fitch_steps<false>)<<<blocks, GF_THREADS, lds_sets, s>>>(
				c->d_gb_pack.as<u64>(), W, C, n, c->d_gf_sched.as<uint32_t>(), c->d_gf_steps.as<uint8_t>(), c->d_gf_min.as<uint8_t>());
			HIP_TRY(hipGetLastError());
			prim::exclusive_scan(s, c->d_gf_tmp, rocprim::make_transform_iterator(c->d_gf_steps.as<uint8_t>(), GfByte{}), c->d_gf_off.as<u64>(), (u64)0, (size_t)C + 1,
			                     rocprim::plus<u64>());
			HIP_TRY(hipEventRecord(c->ev[1], s));
			HIP_TRY(hipMemcpyAsync(&total, c->d_gf_off.as<u64>() + C, 8, hipMemcpyDeviceToHost, s));
			HIP_TRY(hipStreamSynchronize(s));
			times.kernel_ms = sbl_elapsed_ms(c, 0, 1);
			SBL_CHECK(total <= gf_env("SBL_TEST_PARSIMONY_MAX_CHANGES", GF_MAX_CHANGES), SBL_ERR_TOO_LARGE, "too many changes: the change list is limited to 2^26 records (1 GiB)");
			c->d_gf_changes.ensure(std::max<size_t>(1, (size_t)total) * sizeof(sbl_parsimony_change));
			ch.resize((size_t)total);
			HIP_TRY(hipEventRecord(c->ev[0], s));
			HIP_TRY(hipMemsetAsync(c->d_gf_counts.p, 0, (size_t)ne * 16 * 8, s));
			(partial ? k_fitch_changes<true> : k_fitch_changes<false>)<<<blocks, GF_THREADS, lds_all, s>>>(
				c->d_gb_pack.as<u64>(), W, C, n, c->d_gf_sched.as<uint32_t>(), c->d_gf_off.as<u64>(), total, c->d_gf_changes.as<ulonglong2>(),
				c->d_gf_counts.as<unsigned long long>());
			HIP_TRY(hipGetLastError());
			HIP_TRY(hipEventRecord(c->ev[1], s));
			HIP_TRY(hipMemcpyAsync(counts.data(), c->d_gf_counts.p, (size_t)ne * 16 * 8, hipMemcpyDeviceToHost, s));
			HIP_TRY(hipMemcpyAsync(st.data(), c->d_gf_steps.p, (size_t)C, hipMemcpyDeviceToHost, s));
			HIP_TRY(hipMemcpyAsync(mn.data(), c->d_gf_min.p, (size_t)C, hipMemcpyDeviceToHost, s));
			if (total) HIP_TRY(hipMemcpyAsync(ch.data(), c->d_gf_changes.p, (size_t)total * sizeof(sbl_parsimony_change), hipMemcpyDeviceToHost, s));
			HIP_TRY(hipEventRecord(c->ev[2], s));
			HIP_TRY(hipStreamSynchronize(s));
			times.kernel_ms += sbl_elapsed_ms(c, 0, 1);
			times.copy_ms = sbl_elapsed_ms(c, 1, 2);
		}
		c->gf_counts.swap(counts); c->gf_steps.swap(st); c->gf_min.swap(mn); c->gf_changes.swap(ch);
		c->gf_times = times;
		c->stats.device_bytes = sbl_devbuf_total().load();
		*edge_counts = c->gf_counts.data();
		*steps = c->gf_steps.data();
		*minsteps = c->gf_min.data();
		*changes = c->gf_changes.data();
		*nchanges = c->gf_changes.size();
	});
}

extern "C" sbl_status sbl_group_parsimony_times(const sbl_ctx *c, double *kernel_ms, double *copyback_ms)
{
	return sbl_times_out(c, &sbl_ctx::gf_times, kernel_ms, copyback_ms);
}
