// boundary_align.hip -- Postprocessor::ImproveBlockBoundaries (reference src/postprocessor.cpp:156-348), the --correctboundaries step of
// the reference's main (src/sibelia.cpp:198-225, :295-298): every block that occurs once in the reference set (the records of the first
// input file) and once outside it has both instances re-cut by two local alignments of the windows around their starts and ends.
//
// The alignment is SeqAn 1.3.1's localAlignment(align, Score<int>(25, -75, -75)) (src/include/seqan/align/align_local_dynprog.h:229-336,
// :545-648, :718-751).  The matrix is filled from the ends -- M[i][j] is the best score of an alignment STARTING at a[i], b[j]:
//   M[n][*] = M[*][m] = 0;  a[i] == b[j]: M = M[i+1][j+1] + 25 (no comparison against gaps);  otherwise
//   M = max(0, M[i+1][j+1] - 75, max(M[i+1][j], M[i][j+1]) - 75);  bytes are compared as they are (N == N).
// Every cell is pushed into a heap whose sift-up is strict (src/include/seqan/misc/priority_type_heap.h:239-241), j descending outside
// and i descending inside, so the start cell is the first pushed cell that holds the maximum: the largest j, then the largest i.  A
// maximum of 0 leaves the rows as assigned: (0, n), (0, m).  The trace walks forward from the start cell while M[i][j] != 0, i < n, j < m:
// equal characters step diagonally; otherwise with v = M[i+1][j] - 75, d = M[i+1][j+1] - 75, h = M[i][j+1] - 75 it steps i if
// v >= h || d >= h and j if h > v || d >= v.  The result is (i_begin, i_end), (j_begin, j_end).
//
//   kernel    one workgroup per alignment.  Both windows are gathered into LDS from the original records (a reverse window is read
//             downwards through DNASequence::Translate, sbl_dna.h).  Anti-diagonals d = i + j are swept from n + m - 2 down to 0 with
//             three diagonals of 16-bit scores in LDS (a score is at most 2047 * 25 < 2^16), indexed by i: borders are entries no
//             diagonal ever writes, so they stay 0.  A lane fills 4 consecutive cells of the diagonal and -- since the three
//             neighbours of a cell are exactly what the trace compares later -- decides the trace step right there: 2 bits per cell
//             (0 stop, 1 diagonal, 2 i only, 3 j only), one byte per lane, stored BY DIAGONAL so a wave's bytes are consecutive
//             (at most 1.05 MB per alignment; the offset of a diagonal is a closed form, ba_off).  One barrier per diagonal.
//             Every lane keeps its maximum as ONE key score << 22 | j << 11 | i; the workgroup's maximum key is the reference's
//             start cell, ties included.  The trace (at most 4094 steps) is walked by one wave: lane k fetches the code of
//             (i + k, j + k), the run of diagonal steps is consumed with one ballot -- a round per 64 matches or per gap.
//   schedule  corrections depend on each other: the windows of a group are cut where the neighbouring blocks end NOW.  The host
//             keeps the reference's group order, gives every group the level 1 + max(level of the EARLIER groups it may interact
//             with), launches one batch per level and applies its results before it cuts the next level's windows.  Two groups may
//             interact only if a start of one lies within 2R of an end of the other on the same record (DESIGN.md has the argument).
//             SBL_TEST_CORRECT_SERIAL=1 (a number other than 0): one group per level, the reference's own schedule.
//   memory    a batch is split so that its trace codes stay below a cap (256 MB; SBL_TEST_ALIGN_CAP_KB: test switch); one
//             alignment that does not fit the cap by itself fails with SBL_ERR_OOM.
//
// Where the reference is undefined: start < R with a previous block present (start - R wraps as size_t, src/postprocessor.cpp:209) is
// computed signed here, so the window starts behind the previous block; R == 0 is refused (SBL_ERR_BAD_ARG).  Windows are cut to
// their record (the reference reads beyond it).
#include <algorithm>
#include <cstring>
#include <set>

#include "sbl_align.h"

namespace {

constexpr unsigned BA_THREADS = 512, BA_CELLS = 4, BA_MAXLEN = SBL_ALIGN_MAX_LEN, BA_ALIGN = 256;
constexpr size_t BA_DEFAULT_CAP = (size_t)256 << 20;

struct BaJob {
	u64 src_a, src_b;                // first byte of the window in the sequence buffer
	u64 code_off;                    // first byte of its trace codes
	unsigned na, nb, rev_a, rev_b;   // rev: read downwards and complemented
};

// sum of ceil(l / 4) for l = 1 .. L
__host__ __device__ inline u64 ba_ramp(u64 L) { const u64 a = L / 4, r = L % 4; return (a + 1) * (2 * a + r); }

// bytes of trace codes before diagonal d of an n x m matrix (n, m >= 1): diagonal d' has min(d', n - 1) - max(0, d' - (m - 1)) + 1 cells
// -- 1, 2, ..., p, p, ..., p, p - 1, ..., 1 with p = min(n, m) -- packed 4 to a byte, every diagonal starting a new byte
__host__ __device__ inline u64 ba_off(unsigned d, unsigned n, unsigned m)
{
	const unsigned p = n < m ? n : m, q = n < m ? m : n;
	if (d <= p) return ba_ramp(d);
	const u64 flat = (p + 3) / 4;
	if (d <= q) return ba_ramp(p) + (u64)(d - p) * flat;
	return ba_ramp(p) + (u64)(q - p) * flat + ba_ramp(p - 1) - ba_ramp(n + m - 1 - d);
}
__host__ __device__ inline u64 ba_code_bytes(unsigned n, unsigned m) { return ba_off(n + m - 1, n, m); }

__global__ __launch_bounds__(BA_THREADS) void k_boundary_align(const uint8_t *__restrict__ seq, const BaJob *__restrict__ jobs,
                                                               uint8_t *codes, uint4 *__restrict__ out)
{
	__shared__ uint8_t s_a[BA_MAXLEN + 1], s_b[BA_MAXLEN + 1];
	__shared__ unsigned short s_m[3][BA_MAXLEN + 1 + BA_CELLS + 4];      // [diagonal mod 3][i]; entries no diagonal writes are the borders
	__shared__ u64 s_key[BA_THREADS / 64];
	const BaJob J = jobs[blockIdx.x];
	const int n = (int)J.na, m = (int)J.nb;
	const unsigned tid = threadIdx.x;
	for (int t = tid; t < n; t += BA_THREADS) s_a[t] = strand_base(seq, J.src_a, J.na, (unsigned)t, J.rev_a);
	for (int t = tid; t < m; t += BA_THREADS) s_b[t] = strand_base(seq, J.src_b, J.nb, (unsigned)t, J.rev_b);
	for (unsigned t = tid; t < 3 * (BA_MAXLEN + 1 + BA_CELLS + 4); t += BA_THREADS) (&s_m[0][0])[t] = 0;
	__syncthreads();

	uint8_t *const mycodes = codes + J.code_off;
	u64 best = 0;
	u64 off = ba_code_bytes((unsigned)n, (unsigned)m);
	int cur = (n + m - 2) % 3;                                           // buffer of diagonal d; d + 1 and d + 2 follow cyclically
	for (int d = n + m - 2; d >= 0; d--) {
		const int ilo = d - (m - 1) > 0 ? d - (m - 1) : 0, ihi = d < n - 1 ? d : n - 1;
		const unsigned nq = (unsigned)(ihi - ilo + 1 + (BA_CELLS - 1)) / BA_CELLS;
		off -= nq;                                                        // = ba_off(d, n, m)
		unsigned short *const m0 = s_m[cur];
		const unsigned short *const m1 = s_m[cur == 2 ? 0 : cur + 1], *const m2 = s_m[cur == 0 ? 2 : cur - 1];      // (d + 1) % 3, (d + 2) % 3
		for (unsigned q = tid; q < nq; q += BA_THREADS) {
			const int i0 = ilo + (int)(q * BA_CELLS);
			unsigned code = 0;
#pragma unroll
			for (int c = 0; c < (int)BA_CELLS; c++) {
				const int i = i0 + c;
				if (i > ihi) break;
				const int j = d - i;
				const int v = m1[i + 1], h = m1[i], g = m2[i + 1];          // M[i+1][j], M[i][j+1], M[i+1][j+1]
				int val;
				unsigned step;
				if (s_a[i] == s_b[j]) { val = g + AL_MATCH; step = 1; }
				else {
					const int vv = v - AL_PENALTY, hh = h - AL_PENALTY, gg = g - AL_PENALTY;
					val = vv > hh ? vv : hh;
					val = gg > val ? gg : val;
					if (val <= 0) { val = 0; step = 0; }
					else {
						const bool gv = vv >= hh || gg >= hh, gh = hh > vv || gg >= vv;      // never both false
						step = gv && gh ? 1 : gv ? 2 : 3;
					}
				}
				m0[i] = (unsigned short)val;
				code |= step << (2 * c);
				const u64 key = ((u64)(unsigned)val << 22) | ((u64)(unsigned)j << 11) | (u64)(unsigned)i;
				best = key > best ? key : best;
			}
			mycodes[off + q] = (uint8_t)code;
		}
		cur = cur == 0 ? 2 : cur - 1;
		__syncthreads();
	}

	for (int s = 32; s > 0; s >>= 1) {
		const u64 o = __shfl_xor(best, s);
		best = o > best ? o : best;
	}
	if ((tid & 63) == 0) s_key[tid / 64] = best;
	__threadfence_block();
	__syncthreads();
	if (tid >= 64) return;
	best = 0;
	for (unsigned w = 0; w < BA_THREADS / 64; w++) best = s_key[w] > best ? s_key[w] : best;
	int i = (int)(best & 2047), j = (int)((best >> 11) & 2047);
	const int ib = i, jb = j;
	if ((best >> 22) == 0) {                                              // nothing aligns: the rows stay as assigned
		if (tid == 0) out[blockIdx.x] = make_uint4(0, (unsigned)n, 0, (unsigned)m);
		return;
	}
	for (;;) {
		const int ci = i + (int)tid, cj = j + (int)tid;
		unsigned step = 0;                                                // beyond an end: the trace stops there
		if (ci < n && cj < m) {
			const int d = ci + cj, ilo = d - (m - 1) > 0 ? d - (m - 1) : 0;
			const unsigned rel = (unsigned)(ci - ilo);
			step = (mycodes[ba_off((unsigned)d, (unsigned)n, (unsigned)m) + rel / BA_CELLS] >> (2 * (rel % BA_CELLS))) & 3;
		}
		const u64 other = __ballot(step != 1);
		if (!other) { i += 64; j += 64; continue; }
		const int f = __ffsll((long long)other) - 1;
		const unsigned s = (unsigned)__shfl((int)step, f);
		i += f; j += f;
		if (s == 0) break;
		if (s == 2) i++; else j++;
	}
	if (tid == 0) out[blockIdx.x] = make_uint4((unsigned)ib, (unsigned)i, (unsigned)jb, (unsigned)j);
}

size_t ba_cap()
{
	if (const char *e = getenv("SBL_TEST_ALIGN_CAP_KB")) return (size_t)std::max(1ll, atoll(e)) << 10;
	return BA_DEFAULT_CAP;
}

// n alignments over the sequence buffer d_seq, chunked by the cap on the trace codes; out: 4 values per job.  Adds to c->correct_stats.
void ba_run(sbl_ctx *c, const uint8_t *d_seq, std::vector<BaJob> &jobs, uint32_t *out)
{
	const size_t cap = ba_cap();
	std::vector<BaJob> chunk;
	std::vector<size_t> which;
	std::vector<uint32_t> res;
	for (size_t at = 0; at < jobs.size();) {
		chunk.clear(); which.clear();
		u64 bytes = 0;
		for (; at < jobs.size(); at++) {
			BaJob &j = jobs[at];
			if (j.na == 0 || j.nb == 0) { uint32_t *o = out + 4 * at; o[0] = 0; o[1] = j.na; o[2] = 0; o[3] = j.nb; continue; }
			const u64 need = (ba_code_bytes(j.na, j.nb) + BA_ALIGN - 1) / BA_ALIGN * BA_ALIGN;
			if (need > cap) {
				char b[160]; snprintf(b, sizeof b, "out of memory: the trace codes of one %u x %u alignment (%llu bytes) exceed the cap of %zu bytes", j.na, j.nb, need, cap);
				throw SblError{SBL_ERR_OOM, b};
			}
			if (bytes + need > cap) break;
			j.code_off = bytes;
			bytes += need;
			chunk.push_back(j); which.push_back(at);
			c->correct_stats.cells += (u64)j.na * j.nb;
		}
		if (chunk.empty()) continue;
		al_upload(c, c->d_ba_desc, chunk); c->d_ba_codes.ensure((size_t)bytes); c->d_ba_out.ensure(chunk.size() * 16);
		res.resize(chunk.size() * 4);
		c->correct_stats.kernel_ms += al_timed_launch(c, [&] {
			k_boundary_align<<<(unsigned)chunk.size(), BA_THREADS, 0, c->stream>>>(d_seq, c->d_ba_desc.as<BaJob>(), c->d_ba_codes.as<uint8_t>(), c->d_ba_out.as<uint4>());
		}, res.data(), c->d_ba_out.p, chunk.size() * 16);
		c->correct_stats.launches++;
		c->correct_stats.alignments += chunk.size();
		for (size_t k = 0; k < chunk.size(); k++) memcpy(out + 4 * which[k], &res[4 * k], 16);
	}
	c->stats.device_bytes = sbl_devbuf_total().load();
}

struct Window { int64_t lo, hi; };

// the starts and the ends of the instances on one record, as they stand NOW
struct RecordEdges {
	std::multiset<int64_t> starts, ends;
	void add(const sbl_block &b) { starts.insert((int64_t)b.start); ends.insert((int64_t)b.end); }
	void drop(const sbl_block &b) { starts.erase(starts.find((int64_t)b.start)); ends.erase(ends.find((int64_t)b.end)); }
};

// DetermineLeftProbableBoundaries / DetermineRightProbableBoundaries (src/postprocessor.cpp:199-238) of b in the CURRENT list;
// `same` = the instances on its record.  Only the nearest previous End (<= start) and the nearest next Start (>= end) of the OTHER
// instances matter: two searches instead of the reference's scan of the whole list.
void probable_boundaries(const sbl_block &b, RecordEdges &same, int64_t R, int64_t chr_size, Window &left, Window &right)
{
	const int64_t start = (int64_t)b.start, end = (int64_t)b.end;
	int64_t prev_end = -1, next_start = -1;
	same.drop(b);
	auto e = same.ends.upper_bound(start);
	if (e != same.ends.begin()) prev_end = *--e;
	auto s = same.starts.lower_bound(end);
	if (s != same.starts.end()) next_start = *s;
	same.add(b);
	left.hi = start + R;
	if (prev_end >= 0) left.lo = std::max(prev_end, start - R) + 1;          // signed: see the header comment
	else left.lo = start >= R ? start - R + 1 : 0;
	right.lo = end - R + 1;
	right.hi = next_start >= 0 ? std::min(next_start, end + R) : std::min(end + R, chr_size);
	for (Window *w : {&left, &right}) {                                     // cut to the record
		w->lo = std::min(std::max<int64_t>(w->lo, 0), chr_size);
		w->hi = std::min(std::max(w->hi, w->lo), chr_size);
	}
}

}  // namespace

extern "C" sbl_status sbl_correct_stats(const sbl_ctx *c, sbl_correct_stats_t *out)
{
	if (!c || !out) return SBL_ERR_BAD_ARG;
	*out = c->correct_stats;
	return SBL_OK;
}

extern "C" sbl_status sbl_align_windows(sbl_ctx *c, uint64_t ndesc, const sbl_align_desc *desc, uint32_t *out)
{
	return guarded(c, [&] {
		SBL_CHECK(ndesc == 0 || (desc && out), SBL_ERR_BAD_ARG, "null descriptors or result");
		c->correct_stats = sbl_correct_stats_t{};
		std::vector<uint8_t> text;
		std::vector<BaJob> jobs(ndesc);
		for (uint64_t i = 0; i < ndesc; i++) {
			const sbl_align_desc &d = desc[i];
			SBL_CHECK(d.na <= BA_MAXLEN && d.nb <= BA_MAXLEN, SBL_ERR_BAD_ARG, "a string longer than SBL_ALIGN_MAX_LEN");
			SBL_CHECK((d.na == 0 || d.a) && (d.nb == 0 || d.b), SBL_ERR_BAD_ARG, "null string");
			jobs[i] = BaJob{text.size(), text.size() + d.na, 0, d.na, d.nb, 0, 0};
			text.insert(text.end(), d.a, d.a + d.na);
			text.insert(text.end(), d.b, d.b + d.nb);
		}
		if (!ndesc) return;
		c->d_ba_seq.ensure(text.size() + 1);
		if (!text.empty()) HIP_TRY(hipMemcpyAsync(c->d_ba_seq.p, text.data(), text.size(), hipMemcpyHostToDevice, c->stream));
		HIP_TRY(hipStreamSynchronize(c->stream));                            // `text` is pageable
		ba_run(c, c->d_ba_seq.as<uint8_t>(), jobs, out);
	});
}

extern "C" sbl_status sbl_correct_boundaries(sbl_ctx *c, uint32_t min_block_size, uint32_t n_reference_chr, const char *const *names,
                                             const sbl_block **blocks, uint64_t *n, const char **coords, const char **perms, const char **coverage)
{
	return guarded(c, [&] {
		require_records(c);
		require_blocks(c);                                                  // an empty list is one: nothing is corrected
		require_reference_split(c, n_reference_chr);
		const int64_t R = std::min<int64_t>(min_block_size, 1 << 10);          // MAX_CORRECTION_RANGE, src/postprocessor.cpp:15
		SBL_CHECK(R > 0, SBL_ERR_BAD_ARG, "correction range 0 (minimum block size 0): undefined in the reference");
		sbl_check_blocks(c, c->blocks.data(), c->blocks.size());
		c->correct_stats = sbl_correct_stats_t{};

		// ---- the reference's order: GroupBy(blockList, compareById) (src/postprocessor.cpp:321), then per group the swap and the sign
		std::vector<sbl_block> v = c->blocks;
		sbl_sort_by_id(v);
		std::vector<uint32_t> first;                                       // eligible groups: index of the reference instance (the other one follows)
		for_each_id_run(v, [&](size_t i, size_t j) {
			size_t in_ref = 0;
			for (size_t k = i; k < j; k++) in_ref += v[k].chr < n_reference_chr;
			if (in_ref != 1 || j - i != 2) return;
			if (v[i].chr >= n_reference_chr) std::swap(v[i], v[i + 1]);
			if (v[i].id < 0) { v[i].id = -v[i].id; v[i + 1].id = -v[i + 1].id; }
			first.push_back((uint32_t)i);
		});
		const size_t G = first.size();
		std::vector<RecordEdges> same(c->nchr);                             // instances per record
		for (const sbl_block &b : v) same[b.chr].add(b);

		// ---- levels: group g waits for every EARLIER group one of whose instances has a start within 2R of an end of one of g's
		// (or an end within 2R of a start) on the same record
		std::vector<uint32_t> level(G, 1);
		const char *serial = getenv("SBL_TEST_CORRECT_SERIAL");
		if (serial && atoll(serial) != 0) for (size_t g = 0; g < G; g++) level[g] = (uint32_t)g + 1;
		else {
			struct Point { uint32_t chr; int64_t at; uint32_t group; };
			std::vector<Point> starts, ends;
			for (uint32_t g = 0; g < G; g++)
				for (uint32_t k = first[g]; k < first[g] + 2; k++) { starts.push_back({v[k].chr, (int64_t)v[k].start, g}); ends.push_back({v[k].chr, (int64_t)v[k].end, g}); }
			auto less = [](const Point &a, const Point &b) { return a.chr != b.chr ? a.chr < b.chr : a.at < b.at; };
			std::sort(starts.begin(), starts.end(), less);
			std::vector<std::vector<uint32_t>> earlier(G);
			for (const Point &e : ends) {
				auto it = std::lower_bound(starts.begin(), starts.end(), Point{e.chr, e.at - 2 * R, 0}, less);
				for (; it != starts.end() && it->chr == e.chr && it->at <= e.at + 2 * R; ++it)
					if (it->group != e.group) earlier[std::max(it->group, e.group)].push_back(std::min(it->group, e.group));
			}
			for (uint32_t g = 0; g < G; g++) for (uint32_t h : earlier[g]) level[g] = std::max(level[g], level[h] + 1);
		}
		uint32_t levels = 0;
		for (uint32_t l : level) levels = std::max(levels, l);
		std::vector<std::vector<uint32_t>> by_level(levels + 1);
		for (uint32_t g = 0; g < G; g++) by_level[level[g]].push_back(g);      // reference order inside a level

		// ---- one batch per level
		std::vector<BaJob> jobs;
		std::vector<Window> win;
		std::vector<uint32_t> res;
		for (uint32_t l = 1; l <= levels; l++) {
			const std::vector<uint32_t> &gs = by_level[l];
			jobs.clear(); win.assign(gs.size() * 4, Window{0, 0});
			for (size_t t = 0; t < gs.size(); t++) {
				BaJob start{}, end{};
				for (int who = 0; who < 2; who++) {                              // 0 reference instance (string a), 1 assembly instance (string b)
					const uint32_t x = first[gs[t]] + who;
					const int64_t size = (int64_t)c->orig_sepidx[v[x].chr + 1] - c->orig_sepidx[v[x].chr] - 1;
					Window &left = win[4 * t + 2 * who], &right = win[4 * t + 2 * who + 1];
					probable_boundaries(v[x], same[v[x].chr], R, size, left, right);
					// GetBoundariesSequence (:240-255): a negative instance starts at its right window, read in reverse direction
					const bool rev = v[x].id < 0;
					const Window &ws = rev ? right : left, &we = rev ? left : right;
					const u64 base = (u64)c->orig_sepidx[v[x].chr] + 1;
					if (!who) { start.src_a = base + ws.lo; start.na = (unsigned)(ws.hi - ws.lo); start.rev_a = rev; end.src_a = base + we.lo; end.na = (unsigned)(we.hi - we.lo); end.rev_a = rev; }
					else { start.src_b = base + ws.lo; start.nb = (unsigned)(ws.hi - ws.lo); start.rev_b = rev; end.src_b = base + we.lo; end.nb = (unsigned)(we.hi - we.lo); end.rev_b = rev; }
				}
				SBL_CHECK(start.na <= BA_MAXLEN && start.nb <= BA_MAXLEN && end.na <= BA_MAXLEN && end.nb <= BA_MAXLEN, SBL_ERR_INTERNAL, "a correction window longer than 2R - 1");
				jobs.push_back(start); jobs.push_back(end);
			}
			res.assign(jobs.size() * 4, 0);
			ba_run(c, c->d_orig_ch.as<uint8_t>(), jobs, res.data());
			for (size_t t = 0; t < gs.size(); t++) {
				const uint32_t *rs = &res[8 * t], *re = rs + 4;                  // start / end alignment: (a begin, a end, b begin, b end)
				for (int who = 0; who < 2; who++) {                              // UpdateBlockBoundaries (:279-293)
					sbl_block &b = v[first[gs[t]] + who];
					const Window &left = win[4 * t + 2 * who], &right = win[4 * t + 2 * who + 1];
					const int64_t start_first = rs[2 * who], end_second = re[2 * who + 1];
					same[b.chr].drop(b);
					if (b.id > 0) { b.start = (uint64_t)(left.lo + start_first); b.end = (uint64_t)(right.lo + end_second); }
					else { b.start = (uint64_t)(left.hi - end_second); b.end = (uint64_t)(right.hi - start_first); }
					same[b.chr].add(b);
				}
			}
		}
		c->correct_stats.groups = G;
		c->correct_stats.levels = levels;
		c->blocks = v;
		sbl_render_reports(c, names);
		if (blocks) *blocks = c->blocks.data();
		if (n) *n = c->blocks.size();
		if (coords) *coords = c->report[0].c_str();
		if (perms) *perms = c->report[1].c_str();
		if (coverage) *coverage = c->report[2].c_str();
	});
}
