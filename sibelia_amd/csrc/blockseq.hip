// blockseq.hip -- OutputGenerator::ListBlocksSequences (reference src/outputgenerator.cpp:287-318 with OutputLines :102-113): the text of
// blocks_sequences.fasta, spelled on the device from the ORIGINAL records (d_orig_ch, kept since sbl_load / sbl_load_fasta).
//
// This is the one report whose size scales with the input -- every block instance is written out base by base -- and the host never
// holds the parsed records after sbl_load_fasta, so the text is produced where the sequences are.
//
//   host    the reference's order (one unstable std::sort by |id| of a copy of the list: the same libstdc++ call on the same element
//           order, postprocess.hip's group_by / ById), the header lines as one blob, the text length of every instance
//           (header + L + (L ? (L - 1) / 80 : 0) + 1) and their 64-bit exclusive offsets; descriptors and offsets go up once
//   kernel  output-stationary: a lane owns one 16-byte-aligned 16-byte piece of the text and writes it with ONE vector store; a
//           workgroup owns BS_SPAN contiguous bytes, finds the first and last instance of its span by binary search over the text
//           offsets and keeps their descriptors in LDS.  A lane whose piece lies inside one instance's bases (all but a few lanes
//           of a long instance) loads the two aligned 16-byte words its bases come from -- neighbouring lanes read neighbouring
//           words, ascending for a forward and descending for a reverse instance, so the wave's reads stay coalesced either way --
//           and shifts, reverses and complements them in registers; `line = off / 81, col = off % 81` is derived once per lane.
//           The remaining lanes (headers, instance boundaries, instances of a few bases) step byte by byte.
//   back    through a pinned staging buffer owned by the context (pageable when pinning fails, as sbl_get_state does).
#include <algorithm>
#include <cstring>

#include "sbl_ctx.h"
#include "sbl_dna.h"
#include "sbl_text.h"

namespace {

constexpr unsigned BS_THREADS = 256, BS_SPAN = BS_THREADS * 16, BS_LDS = 128;

struct BsDesc {
	unsigned long long src;          // element index of the instance's first base (start) in d_orig_ch
	unsigned long long hoff;         // header line in the header blob
	unsigned L, hlen, rev, pad_;
};

// DNASequence::Translate (src/dnasequence.cpp:11-28) on 8 bytes at once: A <-> T and C <-> G in either case, every other byte unchanged.
__device__ inline u64 complement8(u64 x)
{
	const u64 f = x & 0xDFDFDFDFDFDFDFDFull;                            // case folded: 0x41 only for 'A' / 'a', ...
	const u64 at = (zero8(f ^ 0x4141414141414141ull) | zero8(f ^ 0x5454545454545454ull)) >> 7;
	const u64 cg = (zero8(f ^ 0x4343434343434343ull) | zero8(f ^ 0x4747474747474747ull)) >> 7;
	return x ^ (at * 0x15) ^ (cg * 0x04);                               // 'A' ^ 'T' = 0x15, 'C' ^ 'G' = 0x04
}

__global__ __launch_bounds__(BS_THREADS) void k_block_sequences(const uint8_t *__restrict__ orig, const BsDesc *__restrict__ desc,
                                                                const u64 *__restrict__ toff /* n + 1 */, unsigned long long n,
                                                                const char *__restrict__ headers, u64 total, uint4 *__restrict__ out)
{
	__shared__ BsDesc s_desc[BS_LDS];
	__shared__ u64 s_off[BS_LDS + 1];
	__shared__ unsigned s_first, s_count;
	const u64 span0 = (u64)blockIdx.x * BS_SPAN;
	if (span0 >= total) return;
	const u64 span1 = span0 + BS_SPAN < total ? span0 + BS_SPAN : total;      // one past the last byte of text in the span
	if (threadIdx.x == 0) s_first = bs_find(toff, n, span0);
	if (threadIdx.x == 1) s_count = bs_find(toff, n, span1 - 1);
	__syncthreads();
	const unsigned first = s_first, count = s_count - first + 1;
	__syncthreads();
	// every instance text is at least a header line long, so a span holds few of them; a list that defeats that (it cannot with the
	// reference's header, 44 bytes at least) is served from global memory instead
	const bool in_lds = count <= BS_LDS;
	if (in_lds) {
		for (unsigned i = threadIdx.x; i < count; i += BS_THREADS) s_desc[i] = desc[first + i];
		for (unsigned i = threadIdx.x; i <= count; i += BS_THREADS) s_off[i] = toff[first + i];
		__syncthreads();
	}
	const BsDesc *D = in_lds ? s_desc : desc + first;
	const u64 *O = in_lds ? s_off : toff + first;

	const u64 t0 = span0 + (u64)threadIdx.x * 16;
	if (t0 >= span1) return;
	unsigned di = bs_find(O, count, t0);
	BsDesc d = D[di];
	u64 off = t0 - O[di];                                                 // offset inside the instance's text
	const u64 body = (u64)d.L + (d.L ? (d.L - 1) / 80 : 0);               // bases + inner line breaks
	B16 w;
	if (off >= d.hlen && off + 16 <= d.hlen + body) {
		// ---- the whole piece is bases (and at most one line break) of one instance
		const u64 bo = off - d.hlen;
		const u64 line = bo / 81;
		const unsigned col = (unsigned)(bo % 81);
		const unsigned nl = col >= 65 ? 80 - col : 16;                    // where the line break falls in the piece (16: nowhere)
		const u64 base = line * 80 + col;                                  // first base of the piece (col = 80: the one after the break)
		if (!d.rev) {
			const u64 s0 = d.src + base;
			const uint4 *p = reinterpret_cast<const uint4 *>(orig + (s0 & ~15ull));
			w = window16(p[0], p[1], (unsigned)(s0 & 15));
		} else {
			// bases s0, s0 - 1, ..., s0 - 15: the 16 bytes ending at s0, reversed and complemented
			const u64 s0 = d.src + d.L - 1 - base, a0 = s0 - 15;              // a0 >= d.src - 1 >= 0: at least 14 more bases follow in the piece
			const uint4 *p = reinterpret_cast<const uint4 *>(orig + (a0 & ~15ull));
			const B16 f = window16(p[0], p[1], (unsigned)(a0 & 15));
			w.lo = complement8(__builtin_bswap64(f.hi));
			w.hi = complement8(__builtin_bswap64(f.lo));
		}
		if (nl < 16) w = insert_newline(w, nl);
	} else {
		// ---- headers, boundaries between instances, short instances: byte by byte, (line, col) stepped
		w.lo = w.hi = 0;
		u64 tlen = O[di + 1] - O[di];
		u64 bo = 0, base = 0; unsigned col = 0; bool in_body = false;
		for (unsigned j = 0; j < 16 && t0 + j < total; j++) {
			if (off == tlen) {                                                // next instance (texts are never empty)
				di++; d = D[di]; off = 0; tlen = O[di + 1] - O[di]; in_body = false;
			}
			unsigned char ch;
			if (off < d.hlen) ch = (unsigned char)headers[d.hoff + off];
			else {
				if (!in_body) { bo = off - d.hlen; col = (unsigned)(bo % 81); base = bo / 81 * 80 + col; in_body = true; }
				if (off + 1 == tlen || col == 80) { ch = '\n'; col = 0; }
				else {
					ch = d.rev ? complement1(orig[d.src + d.L - 1 - base]) : orig[d.src + base];
					base++; col++;
				}
			}
			if (j < 8) w.lo |= (u64)ch << (8 * j); else w.hi |= (u64)ch << (8 * (j - 8));
			off++;
		}
	}
	out[t0 / 16] = make_uint4((unsigned)w.lo, (unsigned)(w.lo >> 32), (unsigned)w.hi, (unsigned)(w.hi >> 32));
}

}  // namespace

// the text of n prepared instances, into c->d_bs_text (padded to 16 bytes); leaves the stream busy
void sbl_blockseq_launch(sbl_ctx *c, const void *d_desc, const void *d_toff, uint64_t n, const char *d_headers, uint64_t total)
{
	const uint64_t groups = (total + BS_SPAN - 1) / BS_SPAN;
	SBL_CHECK(groups < 0x7FFFFFFFull, SBL_ERR_TOO_LARGE, "blocks_sequences text too large");
	k_block_sequences<<<(unsigned)groups, BS_THREADS, 0, c->stream>>>(c->d_orig_ch.as<uint8_t>(), static_cast<const BsDesc *>(d_desc), static_cast<const u64 *>(d_toff), n,
	                                                                 d_headers, total, c->d_bs_text.as<uint4>());
	HIP_TRY(hipGetLastError());
}

// the context's pinned staging buffer for device-made text, at least `bytes` large (pageable when pinning fails)
void sbl_text_staging(sbl_ctx *c, size_t bytes)
{
	if (bytes <= c->h_bs_cap) return;
	c->host_free(c->h_bs_text, c->h_bs_pinned);
	c->h_bs_text = nullptr; c->h_bs_cap = 0;
	const size_t cap = bytes + bytes / 16 + 4096;
	c->h_bs_pinned = hipHostMalloc((void **)&c->h_bs_text, cap) == hipSuccess;
	if (!c->h_bs_pinned) {                                             // a host that cannot pin that much still gets its text
		(void)hipGetLastError();
		c->h_bs_text = (char *)malloc(cap);
		if (!c->h_bs_text) throw SblError{SBL_ERR_OOM, "host staging buffer for device-made text"};
	}
	c->h_bs_cap = cap;
}

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
		// headers, descriptors, offsets
		std::string &hdr = c->bs_headers;
		hdr.clear();
		std::vector<BsDesc> desc(n);
		std::vector<u64> toff(n + 1, 0);
		char num[96];
		for (uint64_t i = 0; i < n; i++) {
			const sbl_block &b = v[i];
			const bool fwd = b.id > 0;
			const u64 from = fwd ? b.start + 1 : b.end, to = fwd ? b.end : b.start + 1, L = b.end - b.start;      // src/blockinstance.cpp:57-75
			BsDesc &d = desc[i];
			d.hoff = hdr.size();
			hdr += ">Seq=\"";
			hdr += names ? names[b.chr] : b.chr < c->fa_names.size() ? c->fa_names[b.chr].c_str() : "";
			snprintf(num, sizeof num, "\",Strand='%c',Block_id=%d,Start=%llu,End=%llu\n", fwd ? '+' : '-', b.id > 0 ? b.id : -b.id, from, to);
			hdr += num;
			d.hlen = (unsigned)(hdr.size() - d.hoff);
			SBL_CHECK(hdr.size() - d.hoff < 0xFFFFFFFFull, SBL_ERR_TOO_LARGE, "record description too long");
			d.src = (u64)c->orig_sepidx[b.chr] + 1 + b.start;
			d.L = (unsigned)L; d.rev = fwd ? 0 : 1; d.pad_ = 0;
			toff[i + 1] = toff[i] + d.hlen + L + (L ? (L - 1) / 80 : 0) + 1;
		}
		const u64 total = toff[n];
		c->bs_len = total;
		c->stats.device_bytes = sbl_devbuf_total().load();
		if (total) {
			hipStream_t s = c->stream;
			const size_t padded = (size_t)((total + 15) / 16 * 16);
			c->d_bs_desc.ensure(n * sizeof(BsDesc)); c->d_bs_off.ensure((n + 1) * 8); c->d_bs_hdr.ensure(hdr.size()); c->d_bs_text.ensure(padded);
			sbl_text_staging(c, padded);
			HIP_TRY(hipMemcpyAsync(c->d_bs_desc.p, desc.data(), n * sizeof(BsDesc), hipMemcpyHostToDevice, s));
			HIP_TRY(hipMemcpyAsync(c->d_bs_off.p, toff.data(), (n + 1) * 8, hipMemcpyHostToDevice, s));
			HIP_TRY(hipMemcpyAsync(c->d_bs_hdr.p, hdr.data(), hdr.size(), hipMemcpyHostToDevice, s));
			HIP_TRY(hipEventRecord(c->ev[0], s));
			sbl_blockseq_launch(c, c->d_bs_desc.p, c->d_bs_off.p, n, c->d_bs_hdr.as<char>(), total);
			HIP_TRY(hipEventRecord(c->ev[1], s));
			HIP_TRY(hipMemcpyAsync(c->h_bs_text, c->d_bs_text.p, padded, hipMemcpyDeviceToHost, s));
			HIP_TRY(hipEventRecord(c->ev[2], s));
			HIP_TRY(hipStreamSynchronize(s));
			float k_ms = 0, d_ms = 0;
			(void)hipEventElapsedTime(&k_ms, c->ev[0], c->ev[1]);
			(void)hipEventElapsedTime(&d_ms, c->ev[1], c->ev[2]);
			c->bs_kernel_ms = k_ms; c->bs_copy_ms = d_ms;
			c->stats.device_bytes = sbl_devbuf_total().load();
		}
		if (text) *text = total ? c->h_bs_text : "";
		if (len) *len = total;
	});
}

extern "C" sbl_status sbl_blocks_sequences_times(const sbl_ctx *c, double *kernel_ms, double *copyback_ms)
{
	if (!c) return SBL_ERR_BAD_ARG;
	if (kernel_ms) *kernel_ms = c->bs_kernel_ms;
	if (copyback_ms) *copyback_ms = c->bs_copy_ms;
	return SBL_OK;
}
