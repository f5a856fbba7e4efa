// tree_nj.hip -- the neighbour joining of a batch of distance matrices (include/sibelia_amd.h): the B + 1 trees of
// --coretree --bootstrap B and of the consensus are B + 1 independent runs of one O(n^3) procedure over a matrix of at most 64 x 64
// doubles, which fits the LDS of a workgroup.  One workgroup joins one matrix; the result is sibelia_amd/tree.py's neighbour_joining bit
// for bit, so that a file does not depend on where its trees were built.
//
//   launch    k_nj_batch, one workgroup per matrix, NJ_THREADS lanes (64 up to 16 files).  The matrix lives in LDS with a row stride of
//             NJ_LD = 72 doubles (36 KiB; 8 rows x 8 consecutive columns then fall into 64 different 8-byte bank pairs), beside the row
//             sums, the live list, the node and the leaf mask of every row.  A row is never moved: `live` lists the rows that are left in
//             compacted order -- the order numpy's delete would leave -- and every sum and every index below is over that order.
//   a step    m rows are left (m = n .. 4).  (a) Row sums: 8 lanes per row, lane k the partial sum r[k] of the rule below, folded by
//             shuffles; lane 0 adds the tail.  (b) The argmin of Q over i < j: a lane walks the cells c = i m + j in ascending order and
//             keeps the first of its smallest, then the key (Q, c) is reduced by shuffles in a wave and through LDS across waves: the
//             smaller Q, among equal Q the smaller c -- numpy's argmin over the row-major matrix.  (c) Lane 0 writes the two edges; lane
//             k < m makes cell k of the new row in a register.  (d) After a barrier the row goes to row and column i, live drops j,
//             lane 0 gives row i its node and mask and writes the split.  Four barriers a step.
//   end       the node of the last three rows, by lane 0.
//   host      every argument is checked before any launch, every cell included (finite, symmetric bit for bit, zero diagonal); matrices go
//             up and edges and splits come back in batches of 64 MiB / (8 n^2) matrices, one launch and one host synchronise per batch.
//             The results live in the context until the next call; the call reads and writes nothing of the sbl_group_* calls.
//
// ARITHMETIC.  float64, every operation rounded once: this unit is compiled with contraction off, so no multiply-add is fused; divisions
// are IEEE divisions.  With a[0 .. m - 1] a row over the live columns, diagonal included:
//   row sum   m < 8: s = 0.0, then s += a[k] left to right.  m >= 8: r[k] = a[k] for k < 8, then r[k] += a[i + k] for i = 8, 16, ..
//             while i < m - m % 8; s = ((r0 + r1) + (r2 + r3)) + ((r4 + r5) + (r6 + r7)); then s += a[k] over the m % 8 tail entries left
//             to right; the sum is 0.0 + s (the reduction starts from +0.0: a sum of -0.0 comes out +0.0).  numpy's order up to m = 128.
//   Q         Q[i][j] = ((double)(m - 2) * D[i][j] - r[i]) - r[j]
//   lengths   li = dij / 2 + (r[i] - r[j]) / (double)(2 (m - 2)), lj = dij - li; li < 0: (0, dij); else lj < 0: (dij, 0)
//   new row   ((D[i][k] + D[j][k]) - dij) / 2 for every k, to row and column i; then D[i][i] = 0
//   the end   ((D01 + D02) - D12) / 2, ((D01 + D12) - D02) / 2, ((D02 + D12) - D01) / 2, each x > 0 ? x : 0.0 (Python's max(0.0, x): never
//             -0.0, which fmax may give)
// Cells are taken as the caller gives them: sums that overflow are outside what the bootstrap makes and give what the rules give.
#include <algorithm>
#include <cstring>

#include "sbl_ctx.h"

#pragma clang fp contract(off)

namespace {

typedef unsigned long long u64;

constexpr unsigned NJ_MAX = 64;                        // files: a leaf mask is one word
constexpr unsigned NJ_LD = NJ_MAX + 8;                 // doubles from one row of the LDS matrix to the next
constexpr unsigned NJ_THREADS = 256, NJ_SMALL_THREADS = 64, NJ_SMALL = 16, NJ_WAVE = 64;
constexpr u64 NJ_BUDGET = 64ull << 20;                 // bytes of matrices on the device per batch
constexpr unsigned NJ_NO_CELL = 0xFFFFFFFFu;

// the smaller key (q, c): the smaller q, among equal q the smaller c
__device__ inline void nj_take(double &q, unsigned &c, double oq, unsigned oc)
{
	if (oq < q || (oq == q && oc < c)) { q = oq; c = oc; }
}

// D: the matrices of the launch, n * n doubles each; edges: 2 n - 3 per matrix; splits: n - 3 per matrix.  blockDim.x: a multiple of 64
__global__ __launch_bounds__(NJ_THREADS) void k_nj_batch(const double *__restrict__ D, unsigned n, sbl_nj_edge *__restrict__ edges, u64 *__restrict__ splits)
{
	__shared__ double sD[NJ_MAX * NJ_LD];
	__shared__ double sR[NJ_MAX], sWq[NJ_THREADS / NJ_WAVE];
	__shared__ u64 sMask[NJ_MAX];
	__shared__ unsigned sId[NJ_MAX], sLive[NJ_MAX], sWc[NJ_THREADS / NJ_WAVE];
	const unsigned t = threadIdx.x, nth = blockDim.x, nwaves = nth / NJ_WAVE;
	const double *const src = D + (u64)blockIdx.x * n * n;
	sbl_nj_edge *const E = edges + (u64)blockIdx.x * (2 * n - 3);
	u64 *const S = splits + (u64)blockIdx.x * (n - 3);
	const u64 full = n == 64 ? ~0ull : (1ull << n) - 1;
	for (unsigned x = t; x < n * n; x += nth) sD[x / n * NJ_LD + x % n] = src[x];
	if (t < n) { sLive[t] = t; sId[t] = t; sMask[t] = 1ull << t; }
	__syncthreads();
	for (unsigned s = 0; s + 3 < n; s++) {
		const unsigned m = n - s, whole = m - m % 8;
		// ---- (a) the row sums, 8 lanes a row
		for (unsigned a0 = 0; a0 < m; a0 += nth / 8) {                          // uniform over the workgroup: the shuffles run in every lane
			const unsigned a = a0 + t / 8, k = t % 8;
			const bool row = a < m;
			const double *const A = sD + (row ? sLive[a] : 0) * NJ_LD;
			double r = 0.0;
			if (row && m >= 8) {
				r = A[sLive[k]];
				for (unsigned i = 8; i < whole; i += 8) r = r + A[sLive[i + k]];
			}
			r = r + __shfl_xor(r, 1, NJ_WAVE);
			r = r + __shfl_xor(r, 2, NJ_WAVE);
			r = r + __shfl_xor(r, 4, NJ_WAVE);
			if (row && k == 0) {
				for (unsigned i = m >= 8 ? whole : 0; i < m; i++) r = r + A[sLive[i]];      // m < 8: r is 0.0 here and this is the whole row
				sR[a] = 0.0 + r;
			}
		}
		__syncthreads();
		// ---- (b) the first of the smallest Q over i < j, row-major
		double bq = __builtin_inf();
		unsigned bc = NJ_NO_CELL;
		const double m2 = (double)(m - 2);
		for (unsigned c = t; c < m * m; c += nth) {
			const unsigned i = c / m, j = c - i * m;
			if (i >= j) continue;
			const double q = (m2 * sD[sLive[i] * NJ_LD + sLive[j]] - sR[i]) - sR[j];
			if (q < bq) { bq = q; bc = c; }
		}
		for (unsigned d = NJ_WAVE / 2; d; d >>= 1) nj_take(bq, bc, __shfl_xor(bq, d, NJ_WAVE), __shfl_xor(bc, d, NJ_WAVE));
		if (t % NJ_WAVE == 0) { sWq[t / NJ_WAVE] = bq; sWc[t / NJ_WAVE] = bc; }
		__syncthreads();
		bq = sWq[0]; bc = sWc[0];
		for (unsigned w = 1; w < nwaves; w++) nj_take(bq, bc, sWq[w], sWc[w]);
		if (bc == NJ_NO_CELL) bc = 1;                                           // no Q below infinity (cells that overflow): cell (0, 1), inside the matrix
		const unsigned i = bc / m, j = bc - i * m, pi = sLive[i], pj = sLive[j];
		const double dij = sD[pi * NJ_LD + pj];
		// ---- (c) the two edges; the new row in registers
		if (t == 0) {
			double li = dij / 2.0 + (sR[i] - sR[j]) / (double)(2 * (m - 2)), lj = dij - li;
			if (li < 0) { li = 0.0; lj = dij; }
			else if (lj < 0) { li = dij; lj = 0.0; }
			E[2 * s] = sbl_nj_edge{n + s, sId[pi], li};
			E[2 * s + 1] = sbl_nj_edge{n + s, sId[pj], lj};
		}
		unsigned q = 0, next = 0;
		double v = 0.0;
		if (t < m) {
			q = sLive[t];
			next = t + 1 < m ? sLive[t + 1] : 0;
			v = ((sD[pi * NJ_LD + q] + sD[pj * NJ_LD + q]) - dij) / 2.0;
		}
		__syncthreads();
		// ---- (d) row and column i, the live list without j, the node of row i
		if (t < m) {
			if (q == pi) v = 0.0;
			sD[pi * NJ_LD + q] = v;
			sD[q * NJ_LD + pi] = v;
			if (t >= j && t + 1 < m) sLive[t] = next;
		}
		if (t == 0) {
			const u64 mk = sMask[pi] | sMask[pj];
			sId[pi] = n + s;
			sMask[pi] = mk;
			S[s] = mk & 1 ? full ^ mk : mk;
		}
		__syncthreads();
	}
	if (t == 0) {
		const unsigned a = sLive[0], b = sLive[1], c = sLive[2], top = n + (n - 3);
		const double ab = sD[a * NJ_LD + b], ac = sD[a * NJ_LD + c], bc = sD[b * NJ_LD + c];
		const double x = ((ab + ac) - bc) / 2.0, y = ((ab + bc) - ac) / 2.0, z = ((ac + bc) - ab) / 2.0;
		sbl_nj_edge *const F = E + 2 * (n - 3);
		F[0] = sbl_nj_edge{top, sId[a], x > 0 ? x : 0.0};
		F[1] = sbl_nj_edge{top, sId[b], y > 0 ? y : 0.0};
		F[2] = sbl_nj_edge{top, sId[c], z > 0 ? z : 0.0};
	}
}

[[noreturn]] void nj_bad_cell(u64 tree, unsigned i, unsigned j, const char *what)
{
	char b[160];
	snprintf(b, sizeof b, "matrix %llu, cell (%u, %u) %s", tree, i, j, what);
	throw SblError{SBL_ERR_BAD_ARG, b};
}

// every cell finite, the matrix symmetric bit for bit, the diagonal 0
void nj_check_cells(const double *D, unsigned n, u64 ntrees)
{
	const u64 expo = 0x7FF0000000000000ull;
	for (u64 tr = 0; tr < ntrees; tr++) {
		const double *const M = D + tr * n * n;
		for (unsigned i = 0; i < n; i++) {
			if (M[i * n + i] != 0.0) nj_bad_cell(tr, i, i, "is not 0: the diagonal of a distance matrix is");      // a NaN is not 0 either
			for (unsigned j = i + 1; j < n; j++) {
				u64 a, b;
				memcpy(&a, M + i * n + j, 8);
				memcpy(&b, M + j * n + i, 8);
				if ((a & expo) == expo) nj_bad_cell(tr, i, j, "is not finite");
				if ((b & expo) == expo) nj_bad_cell(tr, j, i, "is not finite");
				if (a != b) nj_bad_cell(tr, i, j, "differs from its mirror cell: a distance matrix is symmetric bit for bit");
			}
		}
	}
}

}  // namespace

extern "C" sbl_status sbl_nj_batch(sbl_ctx *c, const double *D, uint32_t n, uint32_t ntrees, const sbl_nj_edge **edges, const uint64_t **splits)
{
	return guarded(c, [&] {
		SBL_CHECK(n >= 3, SBL_ERR_BAD_ARG, "neighbour joining takes matrices over three or more files");
		SBL_CHECK(n <= NJ_MAX, SBL_ERR_TOO_LARGE, "neighbour joining on the device takes at most 64 files: the leaves of a node are one 64-bit mask");
		SBL_CHECK(edges && splits, SBL_ERR_BAD_ARG, "null edges or splits");
		SBL_CHECK(D || !ntrees, SBL_ERR_BAD_ARG, "null matrices");
		nj_check_cells(D, n, ntrees);
		const u64 cells = (u64)n * n, ne = 2 * (u64)n - 3, ns = (u64)n - 3;
		hipStream_t s = c->stream;
		c->nj_times = SblTimes{};
		c->nj_edges.assign((size_t)(ntrees * ne), sbl_nj_edge{0, 0, 0.0});
		c->nj_splits.assign((size_t)(ntrees * ns), 0);
		const u64 batch = NJ_BUDGET / (cells * 8);                             // 2048 at 64 files; the edges and splits of a matrix are smaller than it
		if (ntrees) {
			const u64 most = std::min<u64>(batch, ntrees);
			c->d_nj_in.ensure((size_t)(most * cells * 8));
			c->d_nj_edges.ensure((size_t)(most * ne * sizeof(sbl_nj_edge)));
			c->d_nj_splits.ensure((size_t)std::max<u64>(1, most * ns) * 8);
		}
		for (u64 t0 = 0; t0 < ntrees; t0 += batch) {
			const u64 nb = std::min<u64>(batch, ntrees - t0);
			HIP_TRY(hipEventRecord(c->ev[0], s));
			HIP_TRY(hipMemcpyAsync(c->d_nj_in.p, D + t0 * cells, (size_t)(nb * cells * 8), hipMemcpyHostToDevice, s));
			HIP_TRY(hipEventRecord(c->ev[1], s));
			k_nj_batch<<<(unsigned)nb, n <= NJ_SMALL ? NJ_SMALL_THREADS : NJ_THREADS, 0, s>>>(c->d_nj_in.as<double>(), n, c->d_nj_edges.as<sbl_nj_edge>(), c->d_nj_splits.as<u64>());
			HIP_TRY(hipGetLastError());
			HIP_TRY(hipEventRecord(c->ev[2], s));
			HIP_TRY(hipMemcpyAsync(c->nj_edges.data() + t0 * ne, c->d_nj_edges.p, (size_t)(nb * ne * sizeof(sbl_nj_edge)), hipMemcpyDeviceToHost, s));
			if (ns) HIP_TRY(hipMemcpyAsync(c->nj_splits.data() + t0 * ns, c->d_nj_splits.p, (size_t)(nb * ns * 8), hipMemcpyDeviceToHost, s));
			HIP_TRY(hipEventRecord(c->ev[3], s));
			HIP_TRY(hipStreamSynchronize(s));
			c->nj_times.kernel_ms += sbl_elapsed_ms(c, 1, 2);
			c->nj_times.copy_ms += sbl_elapsed_ms(c, 0, 1) + sbl_elapsed_ms(c, 2, 3);
		}
		c->stats.device_bytes = sbl_devbuf_total().load();
		*edges = c->nj_edges.data();
		*splits = c->nj_splits.data();
	});
}

extern "C" sbl_status sbl_nj_batch_times(const sbl_ctx *c, double *kernel_ms, double *copy_ms)
{
	return sbl_times_out(c, &sbl_ctx::nj_times, kernel_ms, copy_ms);
}
