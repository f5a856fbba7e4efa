// sbl_ctx.h -- the context behind the C ABI (one per host thread, one GPU each).
#pragma once
#include "sbl_common.h"

// device time of a call's last launch: event pairs around its kernels / around the device-to-host copy of what they made
struct SblTimes { double kernel_ms = 0, copy_ms = 0; };

struct sbl_ctx {
	int device = 0;
	unsigned stage_seq = 0;          // stages run on this context (rotates which launches carry an event pair, simplify.hip)
	hipStream_t stream = nullptr;
	std::string err;
	GlibcRand rng;
	bool tempfile_mode = false;          // sbl_set_tempfile_mode: draw the reference's TempFile names from the stream (see sbl_api.hip)

	// ---- state carried between stages (rawSeq_ / originalPos_, reference src/blockfinder.h:52-54),
	//      resident in HBM as the element array '$' c0 '$' c1 '$' ... '$'
	uint32_t nchr = 0;
	std::vector<uint32_t> sepidx;        // host copy: element index of the '$' before chromosome c (nchr+1)
	size_t nelem = 0;                    // E = L + nchr + 1
	DevBuf d_ch;                         // uint8  [E padded to 32 with '$']
	DevBuf d_op;                         // uint32 [E] original positions (29 bit)
	DevBuf d_sepidx;                     // uint32 [nchr+1]
	// characters the reference would replace through rand() at the next IndexedSequence::Init
	std::vector<uint32_t> amb_elem;      // element indices, chromosome-major order
	std::vector<uint8_t> amb_orig;       // their original characters
	DevBuf d_amb_elem, d_amb_char;
	DevBuf d_fa_text, d_fa_lines, d_fa_recs;   // sbl_load_fasta: file text, per-line and per-record tables
	std::vector<std::string> fa_names;   // record descriptions of the last sbl_load_fasta

	// the records as loaded (originalChrList_): GenerateSyntenyBlocks trims blocks on the ORIGINAL sequences (src/synteny.cpp:36-40)
	DevBuf d_orig_ch;
	std::vector<uint32_t> orig_sepidx;
	sbl_ctx *child = nullptr;            // index over block sequences (TrimBlocks), same device
	void *tiny_out = nullptr;            // mapped host buffer of the small-block index (synteny.hip), hipHostFree'd with the context
	sbl_synteny_stats_t synteny_stats{}; // path counters of the last sbl_generate_blocks
	std::vector<sbl_tiny_result> ti_res; // sbl_tiny_index: what the last call hands out
	std::vector<sbl_inst> ti_inst[2];

	// stage-boundary checkpoint (sbl_save_state / sbl_restore_state)
	DevBuf d_save_ch, d_save_op;
	size_t save_nelem = 0;
	std::vector<uint32_t> save_sepidx, save_amb_elem;
	std::vector<uint8_t> save_amb_orig;
	GlibcRand save_rng;
	bool saved = false;

	// host mirrors for sbl_get_state
	// (copy-back contract of the reference: blockfinder.cpp:85-95).  ONE pinned staging buffer for the whole element array, filled
	// by two bulk device-to-host copies (1 + 4 B per element); the per-chromosome pointers handed out are slices of it.
	bool host_state_valid = false;
	uint8_t *h_ch = nullptr;             // pinned [h_cap] (pageable when the pinned allocation fails: h_pinned)
	uint32_t *h_opos = nullptr;          // pinned [h_cap]
	size_t h_cap = 0;
	bool h_pinned = true;
	// the staging buffer it replaced: pointers handed out by sbl_get_state stay readable (stale, not dangling) for one more
	// generation -- a caller that still holds a slice across a stage + sbl_get_state reads old data instead of freed memory
	uint8_t *h_old_ch = nullptr; uint32_t *h_old_opos = nullptr; bool h_old_pinned = true;
	void host_free(void *p, bool pinned) { if (!p) return; if (pinned) (void)hipHostFree(p); else free(p); }
	void release_host_state()
	{
		host_free(h_ch, h_pinned); host_free(h_opos, h_pinned); host_free(h_old_ch, h_old_pinned); host_free(h_old_opos, h_old_pinned);
		h_ch = h_old_ch = nullptr; h_opos = h_old_opos = nullptr; h_cap = 0;
	}

	// ---- enumeration workspace
	DevBuf d_pk, d_sp;                   // packed bases / separator bits
	DevBuf d_rec_keys[2], d_rec_vals[2]; // k-mer records {mix64(canonical code), element | masks}: position order / partitioned by hash prefix
	DevBuf d_boff;                       // bucket offsets (2^bits + 1)
	DevBuf d_counters;                   // small uint32 scratch block
	DevBuf d_keys, d_payload, d_skeys, d_spayload, d_pairids, d_sorttmp;
	DevBuf d_bif[2];                     // dense marks, uint32 [element capacity]
	DevBuf d_chunkcnt, d_chunkoff, d_scantmp;
	DevBuf d_melem[2], d_mid[2];         // compacted marks per strand (element, id), ascending element
	uint32_t nmarks[2] = {0, 0};
	bool marks_compact_ready = false;    // the enumeration that just ran left d_melem / d_mid / nmarks itself (longk_fp.hip: few members): sbl_compact_marks has nothing to do
	uint32_t bif_count = 0;
	uint32_t cur_k = 0;
	const unsigned long long *dict_keys = nullptr;   // k <= 32: the sorted strand-specific bifurcation codes of the last enumeration (id = rank); nullptr for long k
	DevBuf d_inst;                       // marshalling buffer
	DevBuf d_edges, d_valid;             // sbl_list_edges staging

	// results handed out through the ABI
	std::vector<sbl_inst> inst[2];
	std::vector<sbl_edge> edges;
	std::vector<uint64_t> h_hashes;
	std::vector<sbl_block> blocks;
	bool have_blocks = false;            // sbl_generate_blocks has run: an EMPTY list is a list too
	std::string graph_text;              // sbl_serialize_graph
	std::string report[3];               // sbl_postprocess: blocks_coords.txt, genomes_permutations.txt, coverage_report.txt
	std::string gff_text, coords_text;   // sbl_blocks_gff, sbl_blocks_coords

	// sbl_spell_pieces (spell_text.hip), for sbl_blocks_sequences and sbl_spell_text: descriptors, text offsets, blob of literals and
	// the text on the device; the text comes back through ONE staging buffer (HostText: pinned where that can be had), freed with the
	// context.  The times of the last launch, per entry point
	DevBuf d_bs_desc, d_bs_off, d_bs_hdr, d_bs_text;
	HostText h_bs_text;
	SblTimes bs_times, st_times;

	// sbl_uncovered_calls (uncovered.hip): what it hands out
	std::vector<sbl_uncovered_call> unc_calls;

	// sbl_correct_boundaries / sbl_align_windows (boundary_align.hip): descriptors, trace codes, results, caller-supplied strings
	DevBuf d_ba_desc, d_ba_codes, d_ba_out, d_ba_seq;
	sbl_correct_stats_t correct_stats{};

	// sbl_align_pairs / sbl_align_unique_blocks (block_align.hip): jobs, trace codes, per-job results, runs; the spans and the rows of
	// k_spell_groups (the rows come back through h_bs_text); what the calls hand out
	DevBuf d_ga_job, d_ga_codes, d_ga_out, d_ga_runs, d_ga_span, d_ga_text;
	DevBuf d_ga_score;                   // the global band class: the score arrays of a chunk's pairs, one slice each
	std::vector<sbl_pair_result> ga_res;
	std::vector<sbl_align_run> ga_runs;
	std::vector<sbl_pair_desc> ga_desc;
	std::vector<int32_t> ga_ids;
	sbl_align_stats_t align_stats{};
	uint32_t gap_open = 0;               // sbl_align_set_gap_open: the cost of opening a gap run (0: the linear model of k_block_align, else the affine one)
	uint32_t align_wide = 0;             // sbl_align_set_wide: pairs beyond the LDS band classes run in the global class instead of being skipped
	sbl_align_wide_stats_t wide_stats{}; // ... and what that class did in the last call
	// sbl_align_groups / sbl_align_block_groups: the same pair passes (ga_desc: centre against member); what the calls hand out.  Instances,
	// merged gap slots and groups of k_spell_groups: every sbl_align_* call spells through them, a pair as a group of one member
	DevBuf d_gm_inst, d_gm_slot, d_gm_group;
	std::vector<uint64_t> gm_first;
	std::vector<sbl_group_inst> gm_inst;
	std::vector<sbl_group_result> gm_res;
	std::vector<sbl_member_result> gm_members;
	// The readers of those rows (sbl_groups.h): sbl_group_variants, sbl_group_distances and sbl_group_concat read d_ga_text and
	// d_gm_group / d_gm_slot as the last groups call left them -- valid while gv_rows_valid holds (set by gm_run, cleared wherever those
	// buffers are reused: gm_spell).  They run one after the other on one stream and share what each fills anew: the used groups, the
	// prefix of their padded columns, two counters and the workspace of the compactions.  None of them writes h_bs_text
	bool gv_rows_valid = false;
	DevBuf d_gm_used, d_gm_cbase, d_gm_count, d_gm_tmp;
	// sbl_group_variants (group_variants.hip): class bytes, open / close flags and the compacted columns, segments, slice tables and the
	// packed slices on the device; the slices come back into a host buffer of their own
	DevBuf d_gv_class, d_gv_flag, d_gv_open, d_gv_close, d_gv_seg, d_gv_slice, d_gv_toff, d_gv_text;
	std::vector<sbl_group_segment> gv_segs;
	std::vector<char> gv_text;
	SblTimes gv_times;                   // the kernels / the copy of the slices
	// sbl_group_distances (group_distances.hip): work items, the classes of the instances and the class matrix; the matrix comes back into gd_counts
	DevBuf d_gd_item, d_gd_cls, d_gd_mat;
	std::vector<sbl_pair_counts> gd_counts;
	SblTimes gd_times;                   // clearing the matrix and the kernel / the copy of the matrix
	// sbl_group_concat (group_concat.hip): row starts per (used group, class), first kept column per part, header blob and class text
	// offsets; site flags, compacted columns, sites and the text on the device.  The text comes back through a staging buffer of its
	// own (HostText), freed with the context -- NOT h_bs_text, which holds the rows of the groups call
	DevBuf d_gc_roff, d_gc_first, d_gc_hdr, d_gc_coff, d_gc_flag, d_gc_x, d_gc_site, d_gc_pick, d_gc_text;
	std::vector<sbl_concat_part> gc_parts;
	std::vector<sbl_concat_site> gc_sites;
	HostText h_gc_text;
	SblTimes gc_times;                   // the kernels / the copy of the text
	// sbl_group_bootstrap (group_boot.hip): the packed sites and the count slabs of one batch of replicates; flags, compacted columns and
	// row starts go through sbl_group_concat's d_gc_flag / d_gc_x / d_gc_roff, which every call fills anew.  All slabs come back into gb_counts
	// gp_partial (sbl_group_set_partial): a used group of sbl_group_concat / sbl_group_bootstrap holds every class at most once.  gb_pairs:
	// the clean columns per pair of classes of the last bootstrap call (sbl_group_bootstrap_pairs), folded on the host from d_gb_gclean,
	// one count per used group
	DevBuf d_gb_pack, d_gb_mat, d_gb_gclean;
	std::vector<uint64_t> gb_counts, gb_pairs;
	bool gb_pairs_valid = false;
	uint32_t gp_partial = 0;
	SblTimes gb_times;                   // the kernels of all phases / the copies of the slabs
	// sbl_group_parsimony (group_parsimony.hip) reads d_gb_pack as the last successful sbl_group_bootstrap call left it: no other call
	// writes that buffer, and sbl_group_bootstrap clears gb_pack_valid before it packs anew and sets it, with the classes, the sites and
	// the partial setting of the packed words, where it succeeds.  The schedule of the tree, steps (one byte behind the sites: a 0 for the
	// scan's total), minsteps, offsets, changes and the counts per edge on the device; what the last successful call hands out
	bool gb_pack_valid = false;
	uint32_t gb_pack_nclass = 0, gb_pack_partial = 0;
	uint64_t gb_pack_sites = 0;
	DevBuf d_gf_sched, d_gf_steps, d_gf_min, d_gf_off, d_gf_changes, d_gf_counts, d_gf_tmp;
	std::vector<uint64_t> gf_counts;
	std::vector<uint8_t> gf_steps, gf_min;
	std::vector<sbl_parsimony_change> gf_changes;
	SblTimes gf_times;                   // the two passes and the scan / the copies of the four arrays
	// sbl_nj_batch (tree_nj.hip): the matrices, edges and splits of one batch on the device; the edges and splits of all matrices of the
	// last call.  Nothing here is shared with the sbl_group_* calls
	DevBuf d_nj_in, d_nj_edges, d_nj_splits;
	std::vector<sbl_nj_edge> nj_edges;
	std::vector<uint64_t> nj_splits;
	SblTimes nj_times;                   // the kernels / the uploads of the matrices and the copies of the results
	// sbl_group_mask (group_mask.hip): the prefix of the padded member rows per used group, difference flags, the compacted differences
	// (flat index; row key, centre index, column), start flags and their scan, head / tail flags and the compacted heads and tails, the
	// intervals and their byte ranges, and the masked rows: a buffer of the layout of d_ga_text, valid while gk_valid holds (set by
	// sbl_group_mask, cleared wherever gv_rows_valid is set or cleared).  gk_masked (sbl_group_set_masked): the three readers read
	// it instead of d_ga_text (gm_reader_rows, sbl_groups.h)
	DevBuf d_gk_rbase, d_gk_flag, d_gk_x, d_gk_diff, d_gk_start, d_gk_scan, d_gk_end, d_gk_head, d_gk_tail, d_gk_iv, d_gk_range, d_gk_text;
	std::vector<sbl_mask_interval> gk_intervals;
	SblTimes gk_times;                   // the kernels / the copy of the intervals
	bool gk_valid = false;
	uint32_t gk_masked = 0;

	// ---- multi-GPU enumeration (shard.hip): attached communicator + exchange buffers
	struct SblComm *comm = nullptr;
	DevBuf d_send, d_recv, d_otable, d_oused, d_allkeys, d_allkeys2, d_gelem[2], d_gid[2], d_stage;

	struct LongKScratch *lk = nullptr;   // k > 32 workspace (longk.hip)
	struct LongKFpHolder *lkfp = nullptr;   // k > 32 through window fingerprints (longk_fp.hip)

	// ---- simplification workspace lives in simplify.hip (opaque here)
	struct SimplifyState *simp = nullptr;
	uint32_t window = 0;
	// what an abandoned attempt learnt, carried into the rerun and into later stages (simplify.hip: sbl_simplify_run): the element slack
	// and node capacity a pool overflow asked for, and "the previous stage needed a roll-back: take iteration checkpoints from the start"
	size_t hint_elem_slack = 0, hint_cap_n = 0;
	bool hint_checkpoints = false;

	sbl_stage_stats stats{};
	hipEvent_t ev[8] = {};
};

// every ABI entry point runs under this: no exception crosses the boundary
template <class F>
static sbl_status guarded(sbl_ctx *c, F f)
{
	if (!c) return SBL_ERR_BAD_ARG;
	try {
		(void)hipSetDevice(c->device);
		f();
		return SBL_OK;
	} catch (const SblError &e) {
		c->err = e.msg;
		return e.st;
	} catch (const std::bad_alloc &) {
		c->err = "host allocation failed";
		return SBL_ERR_OOM;
	} catch (...) {
		c->err = "unexpected exception";
		return SBL_ERR_INTERNAL;
	}
}

// milliseconds between two recorded and completed events of the context
inline float sbl_elapsed_ms(sbl_ctx *c, int a, int b)
{
	float ms = 0;
	HIP_TRY(hipEventElapsedTime(&ms, c->ev[a], c->ev[b]));
	return ms;
}

// the body of every sbl_*_times entry point
inline sbl_status sbl_times_out(const sbl_ctx *c, SblTimes sbl_ctx::*t, double *kernel_ms, double *copyback_ms)
{
	if (!c) return SBL_ERR_BAD_ARG;
	if (kernel_ms) *kernel_ms = (c->*t).kernel_ms;
	if (copyback_ms) *copyback_ms = (c->*t).copy_ms;
	return SBL_OK;
}

// what the entry points that read the original records / the context's block list ask for first
inline void require_records(const sbl_ctx *c)
{
	SBL_CHECK(c->orig_sepidx.size() == (size_t)c->nchr + 1 && c->d_orig_ch.p, SBL_ERR_BAD_ARG, "no records loaded");
}
inline void require_blocks(const sbl_ctx *c)      // an empty list is one
{
	SBL_CHECK(c->have_blocks, SBL_ERR_BAD_ARG, "no block list: run sbl_generate_blocks / sbl_postprocess first");
}

// implemented in sbl_api.hip
void sbl_pack(sbl_ctx *c);
void sbl_run_enumeration(sbl_ctx *c, uint32_t k, size_t elem_capacity);   // fills d_bif[0..1], bif_count
void sbl_compact_marks(sbl_ctx *c, int strand);
// implemented in fasta_load.hip
void sbl_finish_load(sbl_ctx *c);   // d_ch / sepidx in place: original positions + list of non-ACGT elements, on the device
// implemented in shard.hip
void sbl_run_enumeration_sharded(sbl_ctx *c, uint32_t k, size_t elem_capacity);   // k <= 32, c->comm attached: hash-prefix sharded table
void sbl_comm_release(sbl_ctx *c);
// implemented in longk.hip
void sbl_run_enumeration_longk(sbl_ctx *c, uint32_t k, size_t elem_capacity);   // k > 32: exact rank doubling
void sbl_run_enumeration_longk_sharded(sbl_ctx *c, uint32_t k, size_t elem_capacity);   // ... split over the GPUs of c->comm
void sbl_longk_free(sbl_ctx *c);
// implemented in longk_fp.hip
bool sbl_run_enumeration_longk_fp(sbl_ctx *c, uint32_t k, size_t elem_capacity);   // k > 32: window fingerprints + bucketed table + exact verification; false = a verification failed, run the doubling
void sbl_longk_fp_free(sbl_ctx *c);
// implemented in postprocess.hip
void sbl_render_reports(sbl_ctx *c, const char *const *names);   // report[0..2] of c->blocks (blocks_coords.txt, genomes_permutations.txt, coverage_report.txt)
void sbl_sort_by_id(std::vector<sbl_block> &v);   // the one unstable sort by |id| the reference's writers apply to a copy of the list
// implemented in blockseq.hip
void sbl_check_blocks(const sbl_ctx *c, const sbl_block *b, uint64_t n);   // a caller's block list against the loaded records (throws SBL_ERR_BAD_ARG)
// h_bs_text, the staging buffer of device-made text (spell_text.hip, blockseq.hip, block_align.hip), grown to `bytes`
inline void sbl_text_staging(sbl_ctx *c, size_t bytes) { c->h_bs_text.ensure(bytes, "host staging buffer for device-made text"); }
// implemented in simplify.hip
void sbl_simplify_run(sbl_ctx *c, uint32_t k, uint32_t D, uint32_t max_iter, sbl_progress_fn progress, void *user, uint64_t *bulges);
void sbl_simplify_free(sbl_ctx *c);
