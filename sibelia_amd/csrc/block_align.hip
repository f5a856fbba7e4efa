// block_align.hip -- base-by-base alignment of the two instances of every unique block: the step the reference's comparison tool
// C-Sibelia.py (reference src/csibelia/C-Sibelia.py:274-309) leaves to one external LAGAN process per block.  The alignment is defined by
// this project (include/sibelia_amd.h): a banded GLOBAL alignment with the scores of sbl_align.h (+25 / -75 / -75,
// 32 bit), filled from the ends so that the trace runs forward, with a certificate that the band lost nothing.
//
//   band      offsets k = j - i - lo + w, 0 <= k < W = |m - n| + 2 w + 1.  On the anti-diagonal d = i + j only the offsets of one
//             parity hold a cell; the three neighbours of a cell are offset k two diagonals back (i + 1, j + 1) and offsets k - 1,
//             k + 1 one diagonal back ((i + 1, j), (i, j + 1)).  So ONE score array indexed by k serves all three diagonals: a diagonal
//             writes its own parity and reads the other one.  Offsets outside [0, W) read as minus infinity; the matrix borders
//             (i == n or j == m) are cells of the sweep with a closed form.
//   model     what the gap costs decide is a type (GaLinear, GaAffine): the score states of a cell (1, or H / E / F), its update and its
//             border form, the bits of a trace code (2 or 4), one round of the trace walk and the limits of the band classes.  A gap
//             opening cost o > 0 (sbl_align_set_gap_open) takes the affine model, o == 0 the linear one; kernel, launcher
//             and pass loop exist once and are instantiated or filled from the model.
//   kernel    k_block_align<M, REG>: one workgroup per pair, diagonals from n + m down to 0.  A lane owns the 8 consecutive offsets
//             8 q .. 8 q + 7: the 4 cells of a diagonal among them give one byte of trace codes (two with the affine model), decided at
//             fill time and stored BY DIAGONAL, so a wave writes consecutive bytes and the offset of a diagonal is d * B.  W <= 512: one
//             wave, the scores live in registers, the neighbours beyond a lane's offsets come by one cross-lane move per state read and
//             side (two per diagonal, four with the affine model), no barrier.  Wider bands: one score array per state in LDS, 256 or
//             M::WIDE_THREADS lanes, one barrier per diagonal.  The bases never fit the LDS as a whole: per 64 diagonals the stretch of
//             a and of b those diagonals touch is staged from the original records (a reverse instance downwards through complement1).
//             Beyond the LDS (sbl_align_set_wide): GaWide<M>, the same sweep with the score arrays in the pair's slice of
//             a device buffer and the bases read from the records; nothing bounds its W.
//   trace     one wave: lane t fetches the code t steps ahead along the direction of the current step, one ballot consumes the run.
//             It emits runs (op, length); the certificate is checked first -- a pair that fails it is not traced.
//   spelling  k_spell_groups, output-stationary like spell_text.hip: a lane owns 16 bytes of the rows, finds its group, its row and its
//             run by binary search over tables the host made from the runs, and writes them with one vector store.  The two gapped
//             rows of a pair are the rows of a group of one member (gm_spell).
//   host      passes: every pending pair runs at its current w; those that miss the certificate double w.  Per pass the pairs are
//             grouped by band class (register / LDS 256 / LDS wide, the limits the model's; with sbl_align_set_wide a fourth, the
//             global one, for the pairs beyond them) and chunked under the total cap on the trace codes.
//   groups    sbl_align_groups / sbl_align_block_groups: a centre-star multiple alignment per group of instances.  Every
//             member against the group's first instance through the same passes (ga_passes); the gap slots of a group merged on the
//             host from the runs; k_spell_groups spells the rows.
#include <algorithm>
#include <cstring>
#include <type_traits>

#include "sbl_groups.h"

namespace {

constexpr int GA_NEG = -(1 << 30);
constexpr int GA_CHUNK = 64;                           // diagonals per staged stretch of bases
constexpr int GA_MAX_STATES = 3;                       // score states of a gap model
constexpr u64 GA_MAX_DIAG = 1ull << 23;                // 75 (n + m) stays clear of GA_NEG
constexpr unsigned GA_W0 = 64;
constexpr size_t GA_PAIR_CAP = (size_t)8 << 30, GA_TOTAL_CAP = (size_t)32 << 30;
constexpr unsigned GA_ALIGN = 256;
constexpr unsigned GA_MAX_OPEN = 100000;               // GA_NEG - o - 75 and -(2 o + 75 (n + m)) stay inside 32 bits

struct GaJob {
	u64 src_a, src_b;                // first byte of the range in the sequence buffer
	u64 code_off, run_off;           // first byte of its trace codes; first run
	unsigned n, m, rev_a, rev_b;
	unsigned w, W, B, full;          // band; offsets; code bytes per diagonal; the band covers the matrix
};
struct GaOut { int score; unsigned nruns, ok, pad_; };

__host__ __device__ inline int ga_bound(int n, int m, int w)
{
	const int mn = n < m ? n : m, diff = n < m ? m - n : n - m;
	return AL_MATCH * (mn - (w + 1)) - AL_PENALTY * (diff + 2 * (w + 1));
}

__device__ inline unsigned ga_seg(unsigned W) { return (W + GA_CHUNK) / 2 + 8; }      // bytes of a staged stretch

// the code of cell (ci, cj), M::CODE_BITS wide; 1 << M::CODE_BITS: beyond the matrix or the band.  The cells of a diagonal lie at every
// second offset, in ascending bits of ascending bytes.
template <class M> __device__ inline unsigned ga_fetch(const uint8_t *codes, const GaJob &J, int lo, int ci, int cj)
{
	constexpr unsigned PER_BYTE = 8 / M::CODE_BITS, NONE = 1u << M::CODE_BITS;
	if (ci >= (int)J.n || cj >= (int)J.m) return NONE;
	const int k = cj - ci - lo + (int)J.w;
	if (k < 0 || k >= (int)J.W) return NONE;
	const unsigned cell = (unsigned)k >> 1;
	return (codes[(u64)(unsigned)(ci + cj) * J.B + cell / PER_BYTE] >> (M::CODE_BITS * (cell % PER_BYTE))) & (NONE - 1);
}

struct GaPos { int i, j, state; };                     // where the trace walk stands; state: the model's own, 0 at the start

// ---- the gap models.  Scores come as arrays over the model's states: dg of (i + 1, j + 1), up of (i + 1, j), lf of (i, j + 1), v the
// cell's own.  UP / LF: bit s set when a cell reads state s of up / lf -- the register path moves only those across lanes.

// linear gap costs: one state, 2 bits of codes (0 diagonal / equal, 1 diagonal / unequal, 2 i step, 3 j step).  LDS
// classes: 4 (W + 2) + 2 (W / 2 + 40) <= 64 KiB
struct GaLinear {
	static constexpr int STATES = 1, CODE_BITS = 2;
	static constexpr unsigned UP = 1, LF = 1;
	static constexpr unsigned REG_W = 512, MID_W = 4096, MAX_W = 12288, WIDE_THREADS = 1024;
	typedef uint8_t Code;                                                   // a lane's 4 cells of a diagonal

	__device__ static unsigned cell(const int (&dg)[1], const int (&up)[1], const int (&lf)[1], bool eq, int, int (&v)[1])
	{
		const int d = dg[0] + (eq ? AL_MATCH : -AL_PENALTY), u = up[0] - AL_PENALTY, l = lf[0] - AL_PENALTY;
		int val = d > u ? d : u;
		val = l > val ? l : val;
		v[0] = val;
		return d == val ? (eq ? 0u : 1u) : u == val ? 2u : 3u;
	}

	// a border cell (i == n or j == m): `rest` gap columns to the end
	__device__ static void border(int rest, bool, bool, int, int (&v)[1]) { v[0] = -AL_PENALTY * rest; }

	// one round of the walk at (i, j): lane t looks t steps ahead along the direction of the first step, one ballot consumes the run
	template <class Emit> __device__ static GaPos walk(const uint8_t *codes, const GaJob &J, int lo, int tid, GaPos at, Emit &emit)
	{
		int i = at.i, j = at.j;
		unsigned c = ga_fetch<GaLinear>(codes, J, lo, i + tid, j + tid);
		const unsigned c0 = (unsigned)__shfl((int)c, 0);
		if (c0 >= 2) c = c0 == 2 ? ga_fetch<GaLinear>(codes, J, lo, i + tid, j) : ga_fetch<GaLinear>(codes, J, lo, i, j + tid);
		const u64 other = __ballot(c != c0);
		const int f = other ? __ffsll((long long)other) - 1 : 64;
		if (c0 < 2) { emit(c0 == 0 ? '=' : 'X', (unsigned)f); i += f; j += f; }
		else if (c0 == 2) { emit('I', (unsigned)f); i += f; }
		else { emit('D', (unsigned)f); j += f; }
		return GaPos{i, j, 0};
	}
};

// a gap opening cost go: H[i][j] the best score of a[i:] against b[j:], E / F the best that starts with a[i] over '-' /
// '-' over b[j]; a gap run of L columns costs go + 75 L.  Codes take 4 bits per cell: bits 0-1 H's choice (0 diagonal / equal, 1
// diagonal / unequal, 2 enter E, 3 enter F), bit 2 "E came by extension" (the run does not close after this column), bit 3 the same for
// F.  Three score arrays in the same 64 KiB of LDS, 12 (W + 2) + 2 (W / 2 + 40) <= 65536: the classes are narrower.
struct GaAffine {
	static constexpr int STATES = 3, CODE_BITS = 4;                         // H, E, F
	static constexpr unsigned UP = 1 | 2, LF = 1 | 4;                       // H, E of (i + 1, j); H, F of (i, j + 1)
	static constexpr unsigned REG_W = 512, MID_W = 2048, MAX_W = 4992, WIDE_THREADS = 640;
	typedef uint16_t Code;                                                  // 256-byte aligned codes, an even B: every 16-bit store is aligned

	__device__ static unsigned cell(const int (&dg)[3], const int (&up)[3], const int (&lf)[3], bool eq, int go, int (&v)[3])
	{
		const int eo = up[0] - go - AL_PENALTY, fo = lf[0] - go - AL_PENALTY, ex = up[1] - AL_PENALTY, fx = lf[2] - AL_PENALTY;
		const int e = ex > eo ? ex : eo, f = fx > fo ? fx : fo;
		const int d = dg[0] + (eq ? AL_MATCH : -AL_PENALTY);
		int val = d > e ? d : e;
		val = f > val ? f : val;
		v[0] = val; v[1] = e; v[2] = f;
		return (d == val ? (eq ? 0u : 1u) : e == val ? 2u : 3u) | (e != eo ? 4u : 0u) | (f != fo ? 8u : 0u);
	}

	// a border cell (i == n or j == m): one gap run of `rest` columns to the end; in_a / in_b: i < n / j < m
	__device__ static void border(int rest, bool in_a, bool in_b, int go, int (&v)[3])
	{
		v[0] = rest ? -go - AL_PENALTY * rest : 0;
		v[1] = in_a ? v[0] : GA_NEG;
		v[2] = in_b ? v[0] : GA_NEG;
	}

	// one round of the walk.  State 0: H -- lane t looks t diagonal steps ahead, one ballot consumes a run of equal codes.  State 1 / 2:
	// inside an I / D run -- lane t looks t columns ahead along i / j; the run closes after the first column whose extension bit is clear.
	template <class Emit> __device__ static GaPos walk(const uint8_t *codes, const GaJob &J, int lo, int tid, GaPos at, Emit &emit)
	{
		int i = at.i, j = at.j, state = at.state;
		if (state == 0) {
			const unsigned x = ga_fetch<GaAffine>(codes, J, lo, i + tid, j + tid), c = x == 16 ? 4 : x & 3;
			const unsigned c0 = (unsigned)__shfl((int)c, 0);
			if (c0 >= 2) return GaPos{i, j, (int)c0 - 1};
			const u64 other = __ballot(c != c0);
			const int len = other ? __ffsll((long long)other) - 1 : 64;
			emit(c0 == 0 ? '=' : 'X', (unsigned)len); i += len; j += len;
		} else {
			const unsigned x = state == 1 ? ga_fetch<GaAffine>(codes, J, lo, i + tid, j) : ga_fetch<GaAffine>(codes, J, lo, i, j + tid);
			const u64 closes = __ballot(x == 16 || !((x >> (state + 1)) & 1));
			int len = closes ? __ffsll((long long)closes) : 64;
			const int room = state == 1 ? (int)J.n - i : (int)J.m - j;
			len = len > room ? room : len;
			emit(state == 1 ? 'I' : 'D', (unsigned)len);
			if (state == 1) i += len; else j += len;
			if (closes) state = 0;
		}
		return GaPos{i, j, state};
	}
};

// the global band class of a model: states, cell, border, codes and walk are M's own; the score arrays lie in the pair's
// slice of a device buffer, not in LDS, and the bases are read from the records, so no limit on W is left.  1024 lanes with either
// model: the class starts above 624 (affine) / 1536 (linear) quads of cells a diagonal, so every lane has a quad on every full diagonal,
// and the 16 waves are what hides the latency of the score loads -- a workgroup has its CU to itself (such pairs are few), and neither
// model's sweep needs more than the 128 VGPRs that size leaves a lane.
template <class M> struct GaWide : M {
	static constexpr bool GLOBAL = true;
	static constexpr unsigned WIDE_THREADS = 1024;
};
template <class M, class = void> struct ga_is_global { static constexpr bool value = false; };
template <class M> struct ga_is_global<M, std::enable_if_t<M::GLOBAL>> { static constexpr bool value = true; };

struct GaView {                                         // what a cell needs to find itself
	int n, m, lo, w, W, imin, jmin, go;
	const uint8_t *sa, *sb;                             // the staged stretches of a and b (from imin / jmin)
	const uint8_t *seq;                                 // the global class: the records, and the job that says where the pair's bases lie in them
	const GaJob *J;
};

// a[i] == b[j]: from the staged stretches; the global class reads the records (neighbouring lanes read neighbouring bytes)
template <class M> __device__ inline bool ga_eq(const GaView &V, int i, int j)
{
	if constexpr (ga_is_global<M>::value)
		return strand_base(V.seq, V.J->src_a, V.J->n, (unsigned)i, V.J->rev_a) == strand_base(V.seq, V.J->src_b, V.J->m, (unsigned)j, V.J->rev_b);
	else return V.sa[i - V.imin] == V.sb[j - V.jmin];
}

// the 4 cells of diagonal d among offsets 8 q + P + 2 c -> their codes.  s: the lane's 8 offsets of every state (REG) -- prev / next:
// s[.][7] of lane q - 1, s[.][0] of lane q + 1
template <class M, int P> __device__ inline unsigned ga_quad_reg(const GaView &V, int d, int q, int *const (&s)[GA_MAX_STATES], const int (&prev)[M::STATES],
                                                                 const int (&next)[M::STATES], int &score)
{
	unsigned bits = 0;
#pragma unroll
	for (int c = 0; c < 4; c++) {
		const int k = 8 * q + 2 * c + P;
		if (k >= V.W) continue;
		const int o = k + V.lo - V.w, i = (d - o) >> 1, j = d - i;
		if (i < 0 || j < 0 || i > V.n || j > V.m) continue;
		int v[M::STATES];
		unsigned code = 0;
		if (i == V.n || j == V.m) M::border((V.n - i) + (V.m - j), i < V.n, j < V.m, V.go, v);
		else {
			const int xu = 2 * c + P - 1 < 0 ? 0 : 2 * c + P - 1, xl = 2 * c + P + 1 > 7 ? 7 : 2 * c + P + 1;
			int dg[M::STATES], up[M::STATES], lf[M::STATES];
#pragma unroll
			for (int t = 0; t < M::STATES; t++) {
				dg[t] = s[t][2 * c + P];
				up[t] = P == 0 && c == 0 ? prev[t] : s[t][xu];
				lf[t] = P == 1 && c == 3 ? next[t] : s[t][xl];
			}
			code = M::cell(dg, up, lf, ga_eq<M>(V, i, j), V.go, v);
		}
#pragma unroll
		for (int t = 0; t < M::STATES; t++) s[t][2 * c + P] = v[t];
		if (d == 0) score = v[0];
		bits |= code << (M::CODE_BITS * c);
	}
	return bits;
}

// the same over the score arrays in memory (LDS, or the pair's slice of the score buffer): state t at S + t (W + 2), S[k + 1] = offset k,
// S[0] and S[W + 1] are minus infinity
template <class M> __device__ inline unsigned ga_quad_mem(const GaView &V, int d, int q, int p, int *S, int &score)
{
	unsigned bits = 0;
#pragma unroll
	for (int c = 0; c < 4; c++) {
		const int k = 8 * q + 2 * c + p;
		if (k >= V.W) break;
		const int o = k + V.lo - V.w, i = (d - o) >> 1, j = d - i;
		if (i < 0 || j < 0 || i > V.n || j > V.m) continue;
		int v[M::STATES];
		unsigned code = 0;
		if (i == V.n || j == V.m) M::border((V.n - i) + (V.m - j), i < V.n, j < V.m, V.go, v);
		else {
			int dg[M::STATES], up[M::STATES], lf[M::STATES];
#pragma unroll
			for (int t = 0; t < M::STATES; t++) {
				const int *X = S + t * (V.W + 2);
				dg[t] = X[k + 1]; up[t] = X[k]; lf[t] = X[k + 2];
			}
			code = M::cell(dg, up, lf, ga_eq<M>(V, i, j), V.go, v);
		}
#pragma unroll
		for (int t = 0; t < M::STATES; t++) S[t * (V.W + 2) + k + 1] = v[t];
		if (d == 0) score = v[0];
		bits |= code << (M::CODE_BITS * c);
	}
	return bits;
}

// M: the gap model; go: its opening cost (the linear model ignores it).  REG: one wave, 8 score registers per state and lane.  Otherwise
// M::STATES arrays of W + 2 scores in LDS and one barrier per diagonal: every cell reads the other parity and writes its own.
// M = GaWide<.>: those arrays in the pair's slice of the score buffer instead -- the host lays a table of the slices' addresses behind the
// job descriptors, so that GaJob and this signature, and with them the code of the LDS and register classes, stay as they were -- nothing staged.  The one barrier per diagonal orders the workgroup's stores
// to its slice against its own later loads as it does in LDS; no other workgroup touches the slice.
template <class M, bool REG> __global__ __launch_bounds__(REG ? 64 : M::WIDE_THREADS) void k_block_align(const uint8_t *__restrict__ seq, const GaJob *__restrict__ jobs, int go,
                                                                                                       uint8_t *codes_all, sbl_align_run *runs_all, GaOut *__restrict__ out)
{
	typedef typename M::Code Code;
	constexpr bool GLOBAL = ga_is_global<M>::value;
	static_assert(8 * sizeof(Code) == 4 * M::CODE_BITS, "a lane's 4 cells of a diagonal are one store");
	static_assert(!(GLOBAL && REG), "the global class has no register form");
	extern __shared__ int ga_lds[];
	__shared__ int s_score;
	const GaJob J = jobs[blockIdx.x];
	const int n = (int)J.n, m = (int)J.m, w = (int)J.w, W = (int)J.W, B = (int)J.B, Q = B / (int)sizeof(Code);      // Q: lanes that hold cells
	const int lo = m - n < 0 ? m - n : 0, omin = lo - w, omax = omin + W - 1;
	const int tid = (int)threadIdx.x, T = (int)blockDim.x;
	int *const S = GLOBAL ? reinterpret_cast<int *const *>(jobs + gridDim.x)[blockIdx.x] : ga_lds;      // LDS and global kernels only
	uint8_t *const sa = reinterpret_cast<uint8_t *>(ga_lds + (REG ? 0 : M::STATES * (W + 2)));
	uint8_t *const sb = sa + ga_seg((unsigned)W);
	uint8_t *const mycodes = codes_all + J.code_off;
	GaView V{n, m, lo, w, W, 0, 0, go, sa, sb, seq, &J};
	// REG: the lane's 8 offsets of state t are s[t][0 .. 7].  One array per state: as a single [STATES][8] object the compiler's resource
	// report shows 78 VGPRs and 6 waves for the affine model instead of 59 and 7.  s[] is a view for the loops over the states: they are
	// unrolled (the pragmas say so), every index is then a constant and the arrays stay in registers.
	static_assert(M::STATES <= GA_MAX_STATES, "a register array per state");
	int s0[8], s1[8], s2[8];
	int *const s[GA_MAX_STATES] = {s0, s1, s2};
	int score = 0;
	if (REG) {
#pragma unroll
		for (int t = 0; t < M::STATES; t++) for (int c = 0; c < 8; c++) s[t][c] = GA_NEG;
	}
	else { for (int k = tid; k < M::STATES * (W + 2); k += T) S[k] = GA_NEG; }
	if (tid == 0) s_score = 0;

	for (int dtop = n + m; dtop >= 0; dtop -= GA_CHUNK) {
		const int dbot = dtop - (GA_CHUNK - 1) > 0 ? dtop - (GA_CHUNK - 1) : 0;
		// the stretch of a and b the cells of diagonals dbot .. dtop read: i = (d - o) / 2, j = (d + o) / 2 over the band's offsets o
		int imin = (dbot - omax) >> 1, imax = (dtop - omin) >> 1, jmin = (dbot + omin) >> 1, jmax = (dtop + omax) >> 1;
		imin = imin < 0 ? 0 : imin; imax = imax > n - 1 ? n - 1 : imax;
		jmin = jmin < 0 ? 0 : jmin; jmax = jmax > m - 1 ? m - 1 : jmax;
		__syncthreads();                                                    // the previous stretch is no longer read; the scores are initialised
		if constexpr (!GLOBAL) {
			for (int t = tid; t <= imax - imin; t += T) sa[t] = strand_base(seq, J.src_a, J.n, (unsigned)(imin + t), J.rev_a);
			for (int t = tid; t <= jmax - jmin; t += T) sb[t] = strand_base(seq, J.src_b, J.m, (unsigned)(jmin + t), J.rev_b);
			V.imin = imin; V.jmin = jmin;
			__syncthreads();
		}
		for (int d = dtop; d >= dbot; d--) {
			const int p = (d - lo + w) & 1;                                  // the parity of the offsets that hold a cell on this diagonal
			Code *const row = reinterpret_cast<Code *>(mycodes + (u64)(unsigned)d * (unsigned)B);
			if (REG) {
				int prev[M::STATES], next[M::STATES];
#pragma unroll
				for (int t = 0; t < M::STATES; t++) {                       // every lane takes part in a move; which moves exist is the model's
					const int below = M::UP >> t & 1 ? __shfl_up(s[t][7], 1) : GA_NEG, above = M::LF >> t & 1 ? __shfl_down(s[t][0], 1) : GA_NEG;
					prev[t] = tid == 0 ? GA_NEG : below;
					next[t] = tid == 63 ? GA_NEG : above;
				}
				const unsigned bits = p ? ga_quad_reg<M, 1>(V, d, tid, s, prev, next, score) : ga_quad_reg<M, 0>(V, d, tid, s, prev, next, score);
				if (tid < Q) row[tid] = (Code)bits;
			} else {
				for (int q = tid; q < Q; q += T) row[q] = (Code)ga_quad_mem<M>(V, d, q, p, S, score);
				__syncthreads();
			}
		}
	}
	// exactly one lane filled (0, 0)
	{
		const int k0 = w - lo, q0 = k0 >> 3;
		if ((REG ? tid : q0 % T) == (REG ? q0 : tid)) s_score = score;
	}
	__threadfence_block();
	__syncthreads();
	if (tid >= 64) return;
	score = s_score;
	if (!J.full && !(score > ga_bound(n, m, w))) {                           // the band may have cut an optimal path: run again, wider
		if (tid == 0) out[blockIdx.x] = GaOut{score, 0, 0, 0};
		return;
	}

	sbl_align_run *const runs = runs_all + J.run_off;
	unsigned nruns = 0, cur_op = 0, cur_len = 0;
	auto emit = [&](unsigned op, unsigned len) {
		if (op == cur_op) { cur_len += len; return; }
		if (cur_len) { if (tid == 0) runs[nruns] = sbl_align_run{cur_op, cur_len}; nruns++; }
		cur_op = op; cur_len = len;
	};
	GaPos at{0, 0, 0};
	while (at.i < n && at.j < m) at = M::walk(mycodes, J, lo, tid, at, emit);
	if (at.i < n) emit('I', (unsigned)(n - at.i));
	if (at.j < m) emit('D', (unsigned)(m - at.j));
	emit(0, 0);
	if (tid == 0) out[blockIdx.x] = GaOut{score, nruns, 1, 0};
}

// ---- spelling: the rows of a centre-star multiple alignment; the two rows of a pair are those of a group of one member

constexpr unsigned GS_THREADS = GM_THREADS;

struct GaSpan { u64 col; unsigned ai, bj, op, len; };                       // a run: first column in its pair's two rows, first base of a / b
struct GmInst { u64 src, first_span; unsigned len, rev, nspans, pad_; };       // a row: its range; a member's spans (of the pair centre / member)

// Output-stationary like spell_text.hip: a lane owns 16 bytes of the text and writes them with one vector store.  Group by binary search
// over text offsets, then row and column; the column's slot by binary search over the group's merged slots, a member's run by binary
// search over its spans by centre index.
// From there the lane steps byte by byte: slot, span, row and group advance as the column does.
__global__ __launch_bounds__(GS_THREADS) void k_spell_groups(const uint8_t *__restrict__ seq, const GmGroup *__restrict__ groups, u64 ngroups,
                                                             const GmInst *__restrict__ insts, const GmSlot *__restrict__ slots,
                                                             const GaSpan *__restrict__ spans, u64 total, uint4 *__restrict__ out)
{
	const u64 t0 = ((u64)blockIdx.x * GS_THREADS + threadIdx.x) * 16;
	if (t0 >= total) return;
	u64 gi = ga_find(0, ngroups, [&](u64 x) { return groups[x].toff <= t0; });
	GmGroup Q = groups[gi];
	u64 off = t0 - Q.toff, row = 0, col = 0, si = 0, xi = 0;
	GmInst I{};
	GmSlot S{};
	u64 next_col = 0;                                                         // where the next slot starts (L: none)
	auto set_slot = [&]() {
		S = slots[Q.first_slot + si];
		next_col = si + 1 < Q.nslots ? slots[Q.first_slot + si + 1].col : Q.L;
	};
	auto seek = [&]() {                                                       // (group, off) -> row, column, slot and span; false: the text is exhausted
		while (off >= (u64)Q.ninst * Q.L) {
			off -= (u64)Q.ninst * Q.L;
			if (++gi >= ngroups) return false;
			Q = groups[gi];
		}
		row = off / Q.L;
		col = off - row * Q.L;
		I = insts[Q.first_inst + row];
		si = gm_slot_at(slots, Q, col);
		set_slot();
		if (row && I.nspans) {
			const unsigned q = (unsigned)gm_centre_before(S, col);            // the centre index this column belongs to
			xi = ga_find(I.first_span, I.first_span + I.nspans, [&](u64 x) { return spans[x].ai <= q; });
		}
		return true;
	};
	u64 wlo = 0, whi = 0;
	bool live = seek();
	for (unsigned b = 0; b < 16 && live && t0 + b < total; b++) {
		if (col == Q.L) { live = seek(); if (!live) break; }
		else if (col == next_col) { si++; set_slot(); }
		const u64 o = col - S.col;
		const bool in_slot = gm_in_slot(S, col);
		const unsigned q = (unsigned)gm_centre_before(S, col);
		unsigned char ch = '-';
		if (row == 0) {
			if (!in_slot) ch = strand_base(seq, I.src, I.len, q, I.rev);
		} else if (I.nspans) {
			while (xi + 1 < I.first_span + I.nspans && spans[xi + 1].ai <= q) xi++;      // the last span that starts at or before centre index q
			GaSpan R = spans[xi];
			long long bj = -1;                                                // the member's base in this column
			if (in_slot) {                                                    // its 'D' run in slot p: R itself (the last run), or the run before R
				if (R.op != 'D' && R.ai == q && xi > I.first_span) R = spans[xi - 1];
				if (R.op == 'D' && R.ai == q && o < R.len) bj = (long long)R.bj + (long long)o;
			} else if (R.op != 'I' && R.op != 'D') bj = (long long)R.bj + (q - R.ai);
			if (bj >= 0) ch = strand_base(seq, I.src, I.len, (unsigned)bj, I.rev);
		}
		if (b < 8) wlo |= (u64)ch << (8 * b); else whi |= (u64)ch << (8 * (b - 8));
		col++; off++;
	}
	store16(out, t0 / 16, B16{wlo, whi});
}

// ---- host

unsigned ga_env(const char *name, unsigned fallback)
{
	if (const char *e = getenv(name)) { const long long v = atoll(e); if (v > 0) return (unsigned)std::min<long long>(v, 1 << 30); }
	return fallback;
}

struct Pending { size_t at; unsigned w; };

constexpr int GA_CLS_GLOBAL = 3;                       // band classes: 0 register, 1 LDS of 256 lanes, 2 LDS wide, 3 global (sbl_align_set_wide)

// the one launch of a chunk of jobs of one band class
template <class M> void ga_launch_cls(sbl_ctx *c, int cls, unsigned blocks, unsigned threads, size_t lds)
{
	const uint8_t *seq = c->d_orig_ch.as<uint8_t>();
	const GaJob *jobs = c->d_ga_job.as<GaJob>();
	const int go = (int)c->gap_open;
	uint8_t *codes = c->d_ga_codes.as<uint8_t>();
	sbl_align_run *runs = c->d_ga_runs.as<sbl_align_run>();
	GaOut *out = c->d_ga_out.as<GaOut>();
	if (cls == 0) k_block_align<M, true><<<blocks, threads, lds, c->stream>>>(seq, jobs, go, codes, runs, out);
	else if (cls == GA_CLS_GLOBAL) k_block_align<GaWide<M>, false><<<blocks, threads, 0, c->stream>>>(seq, jobs, go, codes, runs, out);
	else k_block_align<M, false><<<blocks, threads, lds, c->stream>>>(seq, jobs, go, codes, runs, out);
}

// what the host needs of a gap model
struct GaModel {
	unsigned reg_w, mid_w, max_w;        // the most offsets of the register class, of the LDS class of 256 lanes, of all
	unsigned wide_threads, global_threads;      // lanes of the widest LDS class, of the global class
	unsigned score_bytes, code_bytes;    // bytes of scores per offset; code bytes of a lane's 4 cells of a diagonal
	void (*launch)(sbl_ctx *, int, unsigned, unsigned, size_t);
};
template <class M> GaModel ga_model()
{
	return GaModel{M::REG_W, M::MID_W, M::MAX_W, M::WIDE_THREADS, GaWide<M>::WIDE_THREADS, 4 * M::STATES, sizeof(typename M::Code), ga_launch_cls<M>};
}

// one pass: the pending pairs of one band class at their current w, chunked under the total cap.  Fills res (score, status) and appends
// the runs of the pairs that pass the certificate; returns those that have to run again.
void ga_launch(sbl_ctx *c, const GaModel &model, const std::vector<GaJob> &jobs, const std::vector<size_t> &which, int cls, std::vector<uint8_t> &passed,
               std::vector<uint8_t> &ran_global)
{
	const bool global = cls == GA_CLS_GLOBAL;
	const size_t total_cap = getenv("SBL_TEST_GALIGN_TOTAL_KB") ? (size_t)ga_env("SBL_TEST_GALIGN_TOTAL_KB", 1) << 10 : GA_TOTAL_CAP;
	const unsigned threads = cls == 0 ? 64 : cls == 1 ? 256 : global ? model.global_threads : model.wide_threads;
	std::vector<GaJob> chunk;
	std::vector<GaOut> got;
	std::vector<u64> slice;                                                   // the global class: first score of each job's slice, then its address
	for (size_t at = 0; at < which.size();) {
		chunk.clear(); slice.clear();
		u64 bytes = 0, nrun = 0, nscore = 0, cells = 0;
		size_t lds = 0;
		const size_t first = at;
		for (; at < which.size(); at++) {
			GaJob j = jobs[which[at]];
			const u64 need = ((u64)(j.n + j.m + 1) * j.B + GA_ALIGN - 1) / GA_ALIGN * GA_ALIGN;
			if (!chunk.empty() && bytes + need > total_cap) break;
			j.code_off = bytes; j.run_off = nrun;
			bytes += need; nrun += (u64)j.n + j.m + 1;
			if (global) {                                                     // its slice of the score buffer, kept to whole cache lines
				slice.push_back(nscore);
				nscore += ((u64)(j.W + 2) * model.score_bytes / 4 + 63) / 64 * 64;
				ran_global[which[at]] = 1;
			}
			else lds = std::max(lds, (cls ? (size_t)(j.W + 2) * model.score_bytes : 0) + 2 * (size_t)((j.W + GA_CHUNK) / 2 + 8));
			chunk.push_back(j);
			cells += (u64)(j.n + j.m + 1) * ((j.W + 1) / 2);
		}
		c->d_ga_job.ensure(chunk.size() * (sizeof(GaJob) + sizeof(u64)));
		al_upload(c, c->d_ga_job, chunk); c->d_ga_codes.ensure((size_t)bytes); c->d_ga_out.ensure(chunk.size() * sizeof(GaOut));
		c->d_ga_runs.ensure((size_t)nrun * sizeof(sbl_align_run));
		if (global) {                                                         // the table of slice addresses behind the descriptors
			c->d_ga_score.ensure((size_t)nscore * sizeof(int));
			for (u64 &x : slice) x = (u64)(uintptr_t)(c->d_ga_score.as<int>() + x);
			HIP_TRY(hipMemcpyAsync(c->d_ga_job.as<GaJob>() + chunk.size(), slice.data(), slice.size() * sizeof(u64), hipMemcpyHostToDevice, c->stream));
		}
		got.resize(chunk.size());
		const float ms = al_timed_launch(c, [&] { model.launch(c, cls, (unsigned)chunk.size(), threads, lds); }, got.data(), c->d_ga_out.p, chunk.size() * sizeof(GaOut));
		c->align_stats.kernel_ms += ms;
		c->align_stats.launches++;
		c->align_stats.passes += chunk.size();
		c->align_stats.cells += cells;
		if (global) {
			c->wide_stats.kernel_ms += ms;
			c->wide_stats.launches++;
			c->wide_stats.passes += chunk.size();
			c->wide_stats.cells += cells;
		}
		u64 more = 0;
		for (const GaOut &o : got) more += o.ok ? o.nruns : 0;
		size_t fill = c->ga_runs.size();
		c->ga_runs.resize(fill + (size_t)more);
		for (size_t k = 0; k < chunk.size(); k++) {
			sbl_pair_result &r = c->ga_res[which[first + k]];
			r.passes++;
			r.band_w = chunk[k].w;
			if (!got[k].ok) continue;
			passed[which[first + k]] = 1;
			r.status = SBL_GALIGN_OK; r.score = got[k].score; r.first_run = fill; r.nruns = got[k].nruns;
			if (got[k].nruns) HIP_TRY(hipMemcpyAsync(&c->ga_runs[fill], c->d_ga_runs.as<sbl_align_run>() + chunk[k].run_off, (size_t)got[k].nruns * sizeof(sbl_align_run), hipMemcpyDeviceToHost, c->stream));
			fill += got[k].nruns;
		}
		HIP_TRY(hipStreamSynchronize(c->stream));
	}
}

// the pair passes every sbl_align_* call shares: aligns c->ga_desc (checked) into c->ga_res / ga_runs; jobs: where each pair's bases lie
void ga_passes(sbl_ctx *c, std::vector<GaJob> &jobs)
{
	const std::vector<sbl_pair_desc> &desc = c->ga_desc;
	const size_t N = desc.size();
	const size_t pair_cap = getenv("SBL_TEST_GALIGN_CAP_KB") ? (size_t)ga_env("SBL_TEST_GALIGN_CAP_KB", 1) << 10 : GA_PAIR_CAP;
	const unsigned w0 = ga_env("SBL_TEST_GALIGN_W0", GA_W0);
	const auto from_env = [](unsigned most) { const char *v = getenv("SBL_TEST_GALIGN_WIDE_FROM"); return v ? (unsigned)std::min<long long>(std::max(atoll(v), 0ll), most) : most; };
	// the one place that decides the gap model: a gap opening cost is set (SBL_TEST_GALIGN_AFFINE=1: test switch, sends o == 0 through
	// the affine model as well)
	const char *e = getenv("SBL_TEST_GALIGN_AFFINE");
	const bool affine = c->gap_open > 0 || (e && atoi(e) == 1);
	const GaModel model = affine ? ga_model<GaAffine>() : ga_model<GaLinear>();
	// sbl_align_set_wide: the pairs beyond the widest LDS class (SBL_TEST_GALIGN_WIDE_FROM: test switch, beyond fewer offsets) take the global one
	const unsigned wide_from = from_env(model.max_w);
	c->align_stats = sbl_align_stats_t{};
	c->wide_stats = sbl_align_wide_stats_t{};
	c->align_stats.pairs = N;
	c->ga_res.assign(N, sbl_pair_result{});
	c->ga_runs.clear();
	jobs.assign(N, GaJob{});
	std::vector<Pending> pending;
	for (size_t i = 0; i < N; i++) {
		const sbl_pair_desc &d = desc[i];
		GaJob &j = jobs[i];
		j = GaJob{};
		j.src_a = (u64)c->orig_sepidx[d.chr_a] + 1 + d.start_a; j.src_b = (u64)c->orig_sepidx[d.chr_b] + 1 + d.start_b;
		const u64 n = d.end_a - d.start_a, m = d.end_b - d.start_b;
		sbl_pair_result &r = c->ga_res[i];
		if (n + m >= GA_MAX_DIAG) { r.status = SBL_GALIGN_SKIPPED; continue; }
		j.n = (unsigned)n; j.m = (unsigned)m; j.rev_a = d.rev_a != 0; j.rev_b = d.rev_b != 0;
		if (n == 0 || m == 0) {                                               // all gaps: nothing to fill
			r.score = n + m ? -(int)c->gap_open - AL_PENALTY * (int)(n + m) : 0;
			r.first_run = c->ga_runs.size();
			if (n + m) { c->ga_runs.push_back(sbl_align_run{n ? (uint32_t)'I' : (uint32_t)'D', (uint32_t)(n + m)}); r.nruns = 1; }
			continue;
		}
		pending.push_back(Pending{i, w0});
	}
	std::vector<uint8_t> passed(N, 0), ran_global(N, 0);
	std::vector<size_t> cls[GA_CLS_GLOBAL + 1];
	while (!pending.empty()) {
		for (auto &v : cls) v.clear();
		for (Pending &p : pending) {
			GaJob &j = jobs[p.at];
			const unsigned mn = std::min(j.n, j.m), diff = std::max(j.n, j.m) - mn;
			j.w = std::min(p.w, mn);                                          // w = min(n, m): the band covers the matrix
			j.full = j.w >= mn;
			j.W = diff + 2 * j.w + 1;
			j.B = ((j.W + 1) / 2 + 3) / 4 * model.code_bytes;                 // the lanes that hold cells on a diagonal, each with the codes of its 4
			if ((!c->align_wide && j.W > model.max_w) || (u64)(j.n + j.m + 1) * j.B > pair_cap) { c->ga_res[p.at].status = SBL_GALIGN_SKIPPED; passed[p.at] = 1; continue; }
			cls[c->align_wide && j.W > wide_from ? GA_CLS_GLOBAL : j.W <= model.reg_w ? 0 : j.W <= model.mid_w ? 1 : 2].push_back(p.at);
		}
		for (int k = 0; k <= GA_CLS_GLOBAL; k++) if (!cls[k].empty()) ga_launch(c, model, jobs, cls[k], k, passed, ran_global);
		std::vector<Pending> again;
		for (const Pending &p : pending) if (!passed[p.at]) again.push_back(Pending{p.at, jobs[p.at].w * 2});
		pending.swap(again);
	}
	for (uint8_t g : ran_global) c->wide_stats.pairs += g;
	c->stats.device_bytes = sbl_devbuf_total().load();
}

// the runs of pair i as spans, appended; false: they do not spell its two ranges
bool ga_spans_of(const sbl_ctx *c, size_t i, const GaJob &j, std::vector<GaSpan> &spans)
{
	const sbl_pair_result &r = c->ga_res[i];
	unsigned ai = 0, bj = 0;
	u64 col = 0;
	for (u64 k = 0; k < r.nruns; k++) {
		const sbl_align_run &run = c->ga_runs[r.first_run + k];
		spans.push_back(GaSpan{col, ai, bj, run.op, run.len});
		col += run.len;
		if (run.op != 'D') ai += run.len;
		if (run.op != 'I') bj += run.len;
	}
	return ai == j.n && bj == j.m;
}

struct GmWant { u64 src; unsigned n, rev; size_t pair0, npairs; };          // a group to spell: its centre; its members' pairs, consecutive in c->ga_res
struct GmText { bool ok; u64 L, row_off; };                                 // ok: every pair of the group is aligned -- a group that is not ok has no text

// spells the rows of the groups `want` into h_bs_text and returns the length of the text: per group the merge of the gap slots -- on the
// host, from the runs: they are here already and their number follows the edits, not the bases -- and one launch of k_spell_groups for
// the text of all.  Counts the pairs that are not aligned in align_stats.skipped.
u64 gm_spell(sbl_ctx *c, const std::vector<GaJob> &jobs, const std::vector<GmWant> &want, std::vector<GmText> &text)
{
	std::vector<GmGroup> groups;
	std::vector<GmInst> rows;
	std::vector<GmSlot> slots;
	std::vector<GaSpan> spans;
	std::vector<std::pair<unsigned, unsigned>> runs_d;                          // (slot, length) of the 'D' runs of a group's members
	u64 total = 0;
	c->gv_rows_valid = false;                                                 // the rows and tables sbl_group_variants reads are about to be replaced
	c->gk_valid = false;                                                      // ... and with them what sbl_group_mask made of them
	text.assign(want.size(), GmText{});
	for (size_t g = 0; g < want.size(); g++) {
		const GmWant &w = want[g];
		bool ok = true;
		for (size_t i = w.pair0; i < w.pair0 + w.npairs; i++) if (c->ga_res[i].status != SBL_GALIGN_OK) { ok = false; c->align_stats.skipped++; }
		if (!ok) continue;
		GmGroup Q{total, 0, rows.size(), slots.size(), (unsigned)w.npairs + 1, 0};
		rows.push_back(GmInst{w.src, 0, w.n, w.rev, 0, 0});
		runs_d.clear();
		for (size_t i = w.pair0; i < w.pair0 + w.npairs; i++) {
			const size_t at = spans.size();
			SBL_CHECK(ga_spans_of(c, i, jobs[i], spans), SBL_ERR_INTERNAL, "the runs of an alignment do not spell its two ranges");
			rows.push_back(GmInst{jobs[i].src_b, at, jobs[i].m, jobs[i].rev_b, (unsigned)(spans.size() - at), 0});
			for (size_t x = at; x < spans.size(); x++) if (spans[x].op == 'D') runs_d.push_back({spans[x].ai, spans[x].len});
		}
		std::sort(runs_d.begin(), runs_d.end());                                // by slot, the longest run of a slot last
		u64 shift = 0;
		if (runs_d.empty() || runs_d[0].first != 0) slots.push_back(GmSlot{0, 0, 0});
		for (size_t x = 0; x < runs_d.size(); x++) {
			if (x + 1 < runs_d.size() && runs_d[x + 1].first == runs_d[x].first) continue;
			slots.push_back(GmSlot{runs_d[x].first + shift, runs_d[x].first, runs_d[x].second});
			shift += runs_d[x].second;
		}
		Q.nslots = (unsigned)(slots.size() - Q.first_slot);
		Q.L = (u64)w.n + shift;
		text[g] = GmText{true, Q.L, total};
		total += (u64)Q.ninst * Q.L;
		if (Q.L) groups.push_back(Q);
	}
	if (total) {
		const size_t padded = (size_t)((total + 15) / 16 * 16);
		const unsigned blocks = gm_blocks(padded / 16);
		al_upload(c, c->d_gm_group, groups); al_upload(c, c->d_gm_inst, rows); al_upload(c, c->d_gm_slot, slots); al_upload(c, c->d_ga_span, spans);
		c->d_ga_text.ensure(padded);
		sbl_text_staging(c, padded);
		c->align_stats.spell_ms = al_timed_launch(c, [&] {
			k_spell_groups<<<blocks, GS_THREADS, 0, c->stream>>>(c->d_orig_ch.as<uint8_t>(), c->d_gm_group.as<GmGroup>(), groups.size(), c->d_gm_inst.as<GmInst>(),
			                                                                 c->d_gm_slot.as<GmSlot>(), c->d_ga_span.as<GaSpan>(), total, c->d_ga_text.as<uint4>());
		}, c->h_bs_text.p, c->d_ga_text.p, padded);
		c->stats.device_bytes = sbl_devbuf_total().load();
	}
	return total;
}

// aligns c->ga_desc (checked) into c->ga_res / ga_runs and spells the two rows of every pair, a group of one member, into h_bs_text
void ga_run(sbl_ctx *c, u64 *rows_len)
{
	std::vector<GaJob> jobs;
	ga_passes(c, jobs);
	std::vector<GmWant> want;
	std::vector<GmText> text;
	for (size_t i = 0; i < jobs.size(); i++) want.push_back(GmWant{jobs[i].src_a, jobs[i].n, jobs[i].rev_a, i, 1});
	*rows_len = gm_spell(c, jobs, want, text);
	for (size_t i = 0; i < jobs.size(); i++) {
		sbl_pair_result &r = c->ga_res[i];
		if (text[i].ok) { r.row_off = text[i].row_off; r.row_len = text[i].L; }
		else r = sbl_pair_result{SBL_GALIGN_SKIPPED, 0, r.band_w, r.passes, 0, 0, 0, 0};
	}
}

// aligns the groups c->gm_first / gm_inst (checked) into c->gm_res / gm_members and spells their rows into h_bs_text: every member against
// its centre through the pair passes, then the rows of the groups whose members are all aligned
void gm_run(sbl_ctx *c, u64 *rows_len)
{
	const std::vector<uint64_t> &first = c->gm_first;
	const std::vector<sbl_group_inst> &inst = c->gm_inst;
	const size_t NG = first.size() - 1;
	std::vector<GmWant> want;
	std::vector<GmText> text;
	c->ga_desc.clear();
	for (size_t g = 0; g < NG; g++) {
		const sbl_group_inst &ctr = inst[first[g]];
		want.push_back(GmWant{(u64)c->orig_sepidx[ctr.chr] + 1 + ctr.start, (unsigned)(ctr.end - ctr.start), ctr.rev != 0, c->ga_desc.size(), (size_t)(first[g + 1] - first[g] - 1)});
		for (u64 k = first[g] + 1; k < first[g + 1]; k++)
			c->ga_desc.push_back(sbl_pair_desc{ctr.chr, ctr.start, ctr.end, ctr.rev, inst[k].chr, inst[k].start, inst[k].end, inst[k].rev});
	}
	std::vector<GaJob> jobs;
	ga_passes(c, jobs);
	*rows_len = gm_spell(c, jobs, want, text);

	c->gm_res.assign(NG, sbl_group_result{});
	c->gm_members.assign(inst.size(), sbl_member_result{});
	for (size_t g = 0; g < NG; g++) {
		sbl_group_result &res = c->gm_res[g];
		res.ninst = (uint32_t)(first[g + 1] - first[g]);
		if (text[g].ok) { res.L = text[g].L; res.row_off = text[g].row_off; }
		else res.status = SBL_GALIGN_SKIPPED;
		for (size_t k = 0; k < want[g].npairs; k++) {
			const sbl_pair_result &pr = c->ga_res[want[g].pair0 + k];
			c->gm_members[first[g] + 1 + k] = sbl_member_result{text[g].ok ? pr.score : 0, pr.band_w, pr.passes};
		}
	}
	c->gv_rows_valid = true;                                                  // d_ga_text / d_gm_* hold the rows of these groups until the next gm_spell
	c->gk_valid = false;                                                      // new rows: no mask of them yet (sbl_group_mask)
}

void gm_check(const sbl_ctx *c, u64 ngroups, const uint64_t *first, const sbl_group_inst *inst)
{
	require_records(c);
	SBL_CHECK(ngroups == 0 || (first && inst), SBL_ERR_BAD_ARG, "null group descriptors");
	SBL_CHECK(ngroups == 0 || first[0] == 0, SBL_ERR_BAD_ARG, "the first group does not start at instance 0");
	for (u64 g = 0; g < ngroups; g++) SBL_CHECK(first[g + 1] > first[g], SBL_ERR_BAD_ARG, "an empty group");
	for (u64 i = 0; ngroups && i < first[ngroups]; i++) check_range(c, inst[i].chr, inst[i].start, inst[i].end, "an instance on a record that does not exist");
}

void gm_hand_out(sbl_ctx *c, u64 rows_len, const sbl_group_result **res, const sbl_member_result **members, const char **rows, uint64_t *rl)
{
	if (res) *res = c->gm_res.data();
	if (members) *members = c->gm_members.data();
	if (rows) *rows = rows_len ? c->h_bs_text.p : "";
	if (rl) *rl = rows_len;
}

void ga_check(const sbl_ctx *c, const sbl_pair_desc *d, u64 n)
{
	require_records(c);
	SBL_CHECK(n == 0 || d, SBL_ERR_BAD_ARG, "null pair descriptors");
	for (u64 i = 0; i < n; i++) {
		check_range(c, d[i].chr_a, d[i].start_a, d[i].end_a, "a pair on a record that does not exist");
		check_range(c, d[i].chr_b, d[i].start_b, d[i].end_b, "a pair on a record that does not exist");
	}
}

void ga_hand_out(sbl_ctx *c, u64 rows_len, const sbl_pair_result **res, const sbl_align_run **runs, uint64_t *nruns, const char **rows, uint64_t *rl)
{
	if (res) *res = c->ga_res.data();
	if (runs) *runs = c->ga_runs.data();
	if (nruns) *nruns = c->ga_runs.size();
	if (rows) *rows = rows_len ? c->h_bs_text.p : "";
	if (rl) *rl = rows_len;
}

}  // namespace

extern "C" sbl_status sbl_align_stats(const sbl_ctx *c, sbl_align_stats_t *out)
{
	if (!c || !out) return SBL_ERR_BAD_ARG;
	*out = c->align_stats;
	return SBL_OK;
}

extern "C" sbl_status sbl_align_set_gap_open(sbl_ctx *c, uint32_t open)
{
	return guarded(c, [&] {
		SBL_CHECK(open <= GA_MAX_OPEN, SBL_ERR_BAD_ARG, "a gap opening cost above 100000");
		c->gap_open = open;
	});
}

extern "C" sbl_status sbl_align_get_gap_open(const sbl_ctx *c, uint32_t *open)
{
	if (!c || !open) return SBL_ERR_BAD_ARG;
	*open = c->gap_open;
	return SBL_OK;
}

extern "C" sbl_status sbl_align_set_wide(sbl_ctx *c, uint32_t on)
{
	return guarded(c, [&] {
		SBL_CHECK(on <= 1, SBL_ERR_BAD_ARG, "the wide band setting is 0 or 1");
		c->align_wide = on;
	});
}

extern "C" sbl_status sbl_align_get_wide(const sbl_ctx *c, uint32_t *on)
{
	if (!c || !on) return SBL_ERR_BAD_ARG;
	*on = c->align_wide;
	return SBL_OK;
}

extern "C" sbl_status sbl_align_wide_stats(const sbl_ctx *c, sbl_align_wide_stats_t *out)
{
	if (!c || !out) return SBL_ERR_BAD_ARG;
	*out = c->wide_stats;
	return SBL_OK;
}

extern "C" sbl_status sbl_align_pairs(sbl_ctx *c, uint64_t npairs, const sbl_pair_desc *desc, const sbl_pair_result **res,
                                      const sbl_align_run **runs, uint64_t *nruns, const char **rows, uint64_t *rows_len)
{
	return guarded(c, [&] {
		ga_check(c, desc, npairs);
		c->ga_ids.clear();
		c->ga_desc.assign(desc, desc + npairs);
		u64 total = 0;
		ga_run(c, &total);
		ga_hand_out(c, total, res, runs, nruns, rows, rows_len);
	});
}

extern "C" sbl_status sbl_align_unique_blocks(sbl_ctx *c, uint32_t min_block_size, uint32_t n_reference_chr, const int32_t **ids,
                                              const sbl_pair_desc **desc, uint64_t *n, const sbl_pair_result **res,
                                              const sbl_align_run **runs, uint64_t *nruns, const char **rows, uint64_t *rows_len)
{
	return guarded(c, [&] {
		require_records(c);
		require_blocks(c);
		require_reference_split(c, n_reference_chr);
		sbl_check_blocks(c, c->blocks.data(), c->blocks.size());
		std::vector<sbl_block> v = c->blocks;
		std::stable_sort(v.begin(), v.end(), [](const sbl_block &x, const sbl_block &y) { return std::abs(x.id) < std::abs(y.id); });
		c->ga_ids.clear(); c->ga_desc.clear();
		for_each_id_run(v, [&](size_t i, size_t j) {
			if (j - i != 2 || (v[i].chr < n_reference_chr) == (v[i + 1].chr < n_reference_chr)) return;      // determine_unique_block (C-Sibelia.py:314-323)
			const sbl_block &a = v[i].chr < n_reference_chr ? v[i] : v[i + 1], &b = v[i].chr < n_reference_chr ? v[i + 1] : v[i];
			if (a.end - a.start < min_block_size || b.end - b.start < min_block_size) return;
			c->ga_ids.push_back(std::abs(a.id));
			c->ga_desc.push_back(sbl_pair_desc{a.chr, a.start, a.end, a.id < 0, b.chr, b.start, b.end, b.id < 0});
		});
		u64 total = 0;
		ga_run(c, &total);
		if (ids) *ids = c->ga_ids.data();
		if (desc) *desc = c->ga_desc.data();
		if (n) *n = c->ga_desc.size();
		ga_hand_out(c, total, res, runs, nruns, rows, rows_len);
	});
}

extern "C" sbl_status sbl_align_groups(sbl_ctx *c, uint64_t ngroups, const uint64_t *group_first, const sbl_group_inst *inst,
                                       const sbl_group_result **res, const sbl_member_result **members, const char **rows, uint64_t *rows_len)
{
	return guarded(c, [&] {
		gm_check(c, ngroups, group_first, inst);
		c->ga_ids.clear();
		if (ngroups) { c->gm_first.assign(group_first, group_first + ngroups + 1); c->gm_inst.assign(inst, inst + group_first[ngroups]); }
		else { c->gm_first.assign(1, 0); c->gm_inst.clear(); }
		u64 total = 0;
		gm_run(c, &total);
		gm_hand_out(c, total, res, members, rows, rows_len);
	});
}

extern "C" sbl_status sbl_align_block_groups(sbl_ctx *c, uint32_t min_block_size, const int32_t **ids, const uint64_t **group_first,
                                             const sbl_group_inst **inst, uint64_t *ngroups, const sbl_group_result **res,
                                             const sbl_member_result **members, const char **rows, uint64_t *rows_len)
{
	return guarded(c, [&] {
		require_records(c);
		require_blocks(c);
		sbl_check_blocks(c, c->blocks.data(), c->blocks.size());
		std::vector<sbl_block> v;
		for (const sbl_block &b : c->blocks) if (b.end - b.start >= min_block_size) v.push_back(b);
		// by id, then (chr, start, end, rev): a total order up to identical instances, so the centre does not depend on the sort
		std::sort(v.begin(), v.end(), [](const sbl_block &x, const sbl_block &y) {
			if (std::abs(x.id) != std::abs(y.id)) return std::abs(x.id) < std::abs(y.id);
			if (x.chr != y.chr) return x.chr < y.chr;
			if (x.start != y.start) return x.start < y.start;
			if (x.end != y.end) return x.end < y.end;
			return (x.id < 0) < (y.id < 0);
		});
		c->ga_ids.clear(); c->gm_first.assign(1, 0); c->gm_inst.clear();
		for_each_id_run(v, [&](size_t i, size_t j) {
			if (j - i < 2) return;
			c->ga_ids.push_back(std::abs(v[i].id));
			for (size_t k = i; k < j; k++) c->gm_inst.push_back(sbl_group_inst{v[k].chr, v[k].start, v[k].end, v[k].id < 0});
			c->gm_first.push_back(c->gm_inst.size());
		});
		u64 total = 0;
		gm_run(c, &total);
		if (ids) *ids = c->ga_ids.data();
		if (group_first) *group_first = c->gm_first.data();
		if (inst) *inst = c->gm_inst.data();
		if (ngroups) *ngroups = c->gm_first.size() - 1;
		gm_hand_out(c, total, res, members, rows, rows_len);
	});
}
