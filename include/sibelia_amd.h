/*
 * sibelia_amd.h -- C ABI of the MI355X-native BlockFinder hot path (libsibelia_amd.so).
 *
 * Drop-in boundary for the reference's SyntenyFinder::BlockFinder (bioinf/Sibelia 3.0.7,
 * src/blockfinder.h:28-45).  The reference has no FFI layer; these entry points are what a
 * C++ maintainer binds BlockFinder's methods to (see INTEGRATION.md and
 * include/sibelia_amd/blockfinder.hpp, which restores the reference's class surface on top).
 *
 * Plain pointers and sizes only; no exceptions cross the boundary; every function returns an
 * sbl_status.  One context per host thread; a context owns one GPU (HIP device) and its own
 * glibc-compatible rand() stream (the reference consumes the process-global rand(),
 * src/indexedsequence.cpp:35).
 *
 * All compute runs in HIP kernels on the context's device.  There is no CPU fallback:
 * without a usable gfx950 device sbl_create fails with SBL_ERR_NO_DEVICE.
 */
#ifndef SIBELIA_AMD_H
#define SIBELIA_AMD_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct sbl_ctx sbl_ctx;

typedef enum {
	SBL_OK = 0,
	SBL_ERR_BAD_ARG = 1,       /* k < 2 (stage files enforce k >= 2, src/util.cpp:38-41), null pointers, ... */
	SBL_ERR_NO_DEVICE = 2,     /* no usable HIP device: the product never computes on the host */
	SBL_ERR_OOM = 3,
	SBL_ERR_HIP = 4,           /* HIP runtime error, see sbl_last_error */
	SBL_ERR_TOO_LARGE = 5,     /* a chromosome >= 2^29 bp or total input > 2^30 (src/stranditerator.cpp:19-27, src/common.h:52) */
	SBL_ERR_UNSUPPORTED = 6,   /* vertex size not supported by this build */
	SBL_ERR_INTERNAL = 7
} sbl_status;

/* BlockFinder::State + ProgressCallBack (src/blockfinder.h:31-39): called on the calling thread. */
typedef enum { SBL_PROGRESS_START = 0, SBL_PROGRESS_RUN = 1, SBL_PROGRESS_END = 2 } sbl_progress_state;
typedef void (*sbl_progress_fn)(size_t progress, int state, void *user);

/* BifurcationInstance (src/indexedsequence.h:57-68).  Negative-strand `pos` is in reverse-complement
 * coordinates, exactly as EnumerateBifurcationsSArrayInRAM reports it (src/vertexenumeration.cpp:334-346). */
typedef struct { uint32_t id, chr, pos; } sbl_inst;

/* BlockFinder::Edge (src/blockfinder.h:58-90) as produced by ListEdges (src/serialization.cpp:56-86). */
typedef struct {
	uint32_t chr, strand;            /* strand 0 = positive, 1 = negative */
	uint32_t start_vertex, end_vertex;
	uint32_t pos, len;               /* actual position (+ coordinates) and length */
	uint32_t orig_pos, orig_len;     /* DNASequence::SpellOriginal (src/dnasequence.cpp:254-260) */
	char first_char;
	char pad_[3];
} sbl_edge;

/* Per-stage counters / timings of the last sbl_simplify_stage (times measured on the device). */
typedef struct {
	uint64_t strand_kmers;           /* N = 2 * sum(max(0, len - k + 1)), the metric's unit */
	uint64_t bif_count, instances;   /* after enumeration */
	uint64_t bulges;                 /* return value of PerformGraphSimplifications */
	uint32_t iterations, rounds;     /* SimplifyGraph iterations run; ordered-commit rounds launched */
	uint32_t replays;                /* iterations re-run (order validation fired, or a pool had to grow), + 1 for an abandoned checkpoint-free first attempt */
	uint32_t grow_replays;           /* ... of which because the element / node pool had to grow */
	double enumerate_ms, simplify_ms, copyback_ms, total_ms;
	double kmer_table_ms;            /* duration of the dominant kernel (k-mer table build) */
	uint64_t kmer_table_bytes;       /* its algorithmic HBM bytes */
	double snapshot_ms, reserve_ms, commit_ms;   /* SimplifyGraph kernel time by phase */
	double probe_ms;
	uint64_t executed;               /* pending ids examined in ordered rounds (retired by the probe or committed) */
	uint64_t transactions;           /* ... of which RemoveBulges transactions that owned their neighbourhood and ran */
	double exchange_ms;              /* sharded enumeration: host time inside the collectives (all-to-all + gathers) */
	uint64_t exchange_bytes;         /* ... and the bytes this GPU sent to its peers */
	uint64_t chain_transactions;     /* transactions run by the serial chain (dense conflict neighbourhoods: small k, low complexity) */
	/* probe_ms / reserve_ms / commit_ms come from start stamps the round kernels write themselves (device wall clock, every launch);
	 * HIP event pairs are recorded around every 4th launch of the commit kernel only (an event pair costs ~8 us of barrier packets): */
	double commit_event_ms;          /* sum of those event-pair times */
	uint64_t commit_event_launches;  /* ... and how many launches they cover */
	/* SBL_CHECK_DICTIONARY=1 (k <= 32): the reference's _DEBUG invariant IndexedSequence::Test (src/indexedsequence.cpp:74-103) on the
	 * stage's final graph -- windows whose stored mark was compared with the dictionary of the initial marking, and how many differed
	 * (a stage with mismatches fails with SBL_ERR_INTERNAL) */
	uint64_t dict_checked, dict_mismatches;
	/* read-only simplification phases split over the attached GPUs (snapshots by id range, probes by window share; commits replicated):
	 * GPUs sharing them (1 = not split), host time inside the verdict all-gathers, bytes this GPU sent (1 B per id per snapshot,
	 * 1 B per window entry per round) */
	uint64_t ro_ranks;
	double verdict_ms;
	uint64_t verdict_bytes;
	/* k > 32 (round 6): which enumeration ran -- 0 none (k <= 32), 1 window fingerprints + bucketed table + exact verification
	 * (longk_fp.hip), 2 exact rank doubling on request / on several GPUs (longk.hip), 3 rank doubling after a failed verification --
	 * and the occurrences of bifurcation k-mers that were compared with their group's representative on the sequence (k/4 B each) */
	uint64_t longk_path;
	uint64_t fp_verified;
	/* device memory held by the library's buffers of this PROCESS when the stage ended (grow-only workspaces: the peak so far) */
	uint64_t device_bytes;
} sbl_stage_stats;

/* Replaces: BlockFinder::BlockFinder(chrList[, tempDir]) + Init (src/blockfinder.cpp:53-76).
 * device < 0 selects the current HIP device. */
sbl_status sbl_create(sbl_ctx **out, int device);
void sbl_destroy(sbl_ctx *ctx);

/* Replaces BlockFinder::Init (src/blockfinder.cpp:65-76): sequences are upper-case ASCII as
 * delivered by the reference FASTA reader (src/fasta.cpp:92-104); originalPos = identity.
 * Uploads the state to HBM; inputs are borrowed for the call only. */
sbl_status sbl_load(sbl_ctx *ctx, uint32_t nchr, const uint8_t *const *seq, const uint64_t *len);

/* Upstream of the hot path: replaces FASTAReader::GetSequences (src/fasta.cpp:23-104) + BlockFinder::Init.
 * The file is mapped and copied to the device as text; line splitting, trimming, header / sequence classification,
 * upper-casing, validation ("ACGTURYKMSWBDHWNX-"), concatenation, identity original positions and the scan for non-ACGT
 * characters run in kernels.  Parse errors come back as SBL_ERR_BAD_ARG with the reference's message
 * ("parse error in <file> on line <n>: empty sequence | empty header | illegal character: <c>") in sbl_last_error: the first
 * offending line and, within it, the first offending column, exactly, wherever in the file they lie; <c> is the byte as written.
 * A load that fails leaves the context without records (sbl_nchr 0); one that succeeds leaves sbl_last_error empty.
 * sbl_record_name: FASTARecord::GetDescription (text between '>' and the first blank), valid until the next load. */
sbl_status sbl_load_fasta(sbl_ctx *ctx, const char *path);
const char *sbl_record_name(const sbl_ctx *ctx, uint32_t chr);

/* Replaces IndexedSequence::Init's enumeration (src/indexedsequence.cpp:28-47 ->
 * src/vertexenumeration.cpp:263-364) on the current state at vertex size k.
 * Arrays are owned by the ctx, sorted by (chr,pos), valid until the next call on the ctx. */
sbl_status sbl_enumerate(sbl_ctx *ctx, uint32_t k, uint32_t *bif_count,
                         const sbl_inst **pos, uint64_t *npos, const sbl_inst **neg, uint64_t *nneg);

/* Replaces BlockFinder::PerformGraphSimplifications (src/blockfinder.cpp:78-98): enumeration,
 * marking, SimplifyGraph (bulge removal, src/blockfinder.cpp:16-51, src/bulgeremoval.cpp) and
 * copy-back, all on the device; the state stays resident in HBM. */
sbl_status sbl_simplify_stage(sbl_ctx *ctx, uint32_t k, uint32_t min_branch_size, uint32_t max_iterations,
                              sbl_progress_fn progress, void *user, uint64_t *bulges);

/* rawSeq_[chr] / originalPos_[chr] (src/blockfinder.h:52-54), downloaded on demand.
 * Borrowed pointers, valid until the next mutating call. */
sbl_status sbl_get_state(sbl_ctx *ctx, uint32_t chr, const uint8_t **seq, const uint32_t **orig_pos, uint64_t *len);
uint32_t sbl_nchr(const sbl_ctx *ctx);
/* Length of record chr as loaded (sbl_load or sbl_load_fasta; simplification does not change it); 0 for a record that does not exist. */
uint64_t sbl_record_size(const sbl_ctx *ctx, uint32_t chr);

/* Replaces BlockFinder::ListEdges on a fresh index at k (src/serialization.cpp:56-86), the
 * observation channel behind SerializeCondensedGraph (src/serialization.cpp:88-110). */
sbl_status sbl_list_edges(sbl_ctx *ctx, uint32_t k, const sbl_edge **edges, uint64_t *n);

/* Downstream of the hot path: replaces BlockFinder::GenerateSyntenyBlocks (src/synteny.cpp:229-286, with
 * ResolveOverlap :124-166 and TrimBlocks :31-122; src/blockfinder.h:43) on the current state.  Both indices it needs -- the edge
 * list at k and, per candidate block, a fresh index at trim_k over the block's ORIGINAL sequences (kept on the device since
 * sbl_load / sbl_load_fasta) -- are built by the enumeration kernels; rand() is consumed exactly as the reference does.
 * sbl_block = BlockInstance (src/blockinstance.h:21-47): signed block id (sign = strand), chromosome, [start, end) in original
 * coordinates; sorted by (chr, start) like the reference's result.  Owned by the ctx, valid until the next call. */
typedef struct { int32_t id; uint32_t chr; uint64_t start, end; } sbl_block;
sbl_status sbl_generate_blocks(sbl_ctx *ctx, uint32_t k, uint32_t trim_k, uint32_t min_size, int shared_only,
                               const sbl_block **blocks, uint64_t *n);

/* Which way the candidate blocks of the last sbl_generate_blocks were indexed at trim_k (csrc/synteny.hip): by the small-block
 * kernel -- speculated for a whole chunk of groups in one batch launch, or one block in one launch after a speculation miss and on
 * every further trim iteration -- or by the general child index (gather + the full enumeration).  A block goes to the small-block
 * kernel when it has at most 1024 elements (bases + sequences + 1) in at most 16 sequences and trim_k <= 32; the kernel declines a
 * block that holds a character other than A, C, G, T, which then takes the general path.  Host counters only: they cost no device
 * work and change no result.  With SBL_NO_TINY_INDEX set every small-block counter stays 0. */
typedef struct {
	uint64_t groups_resolved;        /* groups of at least 2 edges with one on the positive strand: those that reach ResolveOverlap */
	uint64_t batch_launches;         /* launches of the batched small-block kernel (one per chunk of groups that queued an index) */
	uint64_t batch_indices;          /* indices queued in those launches */
	uint64_t speculated_used;        /* queued indices that were used: the candidate block came out as speculated and was indexed */
	uint64_t single_launches;        /* launches of the one-block small-block kernel */
	uint64_t batch_declines;         /* queued indices that were consulted and had declined (each is then tried once more by a single launch) */
	uint64_t single_declines;        /* one-block launches that declined */
	uint64_t general_indices;        /* general child indices */
	uint64_t tiny_max_elements;      /* largest block indexed by the small-block kernel (declined ones excluded): elements ... */
	uint64_t tiny_max_records;       /* ... and sequences (each the maximum over those blocks) */
	uint64_t general_max_elements;   /* the same over the blocks that took the general child index */
	uint64_t general_max_records;
	uint64_t tiny_max_keys;          /* largest bifurcation count (both orientations) a small-block index reported */
} sbl_synteny_stats_t;
sbl_status sbl_synteny_stats(const sbl_ctx *ctx, sbl_synteny_stats_t *out);

/* TEST ENTRY POINT: the small-block index on its own -- for every candidate block given, the index at trim_k that
 * sbl_generate_blocks' TrimBlocks would read, built by the same host code and the same kernels (csrc/synteny.hip: batched != 0 queues
 * every eligible block and runs ONE launch of the batched kernel; batched == 0 runs one launch of the one-block kernel per eligible
 * block).  Block b is ranges[block_first[b], block_first[b + 1]) (nblocks + 1 ascending offsets, the first one 0); a range is bases
 * [start, end) of ORIGINAL record chr, whatever stages have run since the load.
 * sbl_tiny_result: status SBL_TINY_INDEXED -- bif_count and the instance lists pos[first_pos, first_pos + npos) and
 * neg[first_neg, first_neg + nneg) are those of sbl_enumerate(trim_k) on the block's sequences as records 0, 1, ..., the negative list
 * with each sequence's run in descending element order like sbl_enumerate's; SBL_TINY_DECLINED -- the kernel met a byte other than
 * A, C, G, T (sbl_generate_blocks then takes the general child index); SBL_TINY_NOT_ELIGIBLE -- no range, more than 16 ranges, more
 * than 1024 elements (bases + ranges + 1) or trim_k > 32: nothing was launched for it.  The last two carry no count and no instances.
 * Every argument is checked on the host before anything is launched.  SBL_ERR_BAD_ARG: trim_k < 2, no records loaded, offsets that do
 * not start at 0 or descend, chr >= sbl_nchr(ctx), an empty range, a range beyond its record.
 * Draws nothing from the rand() stream and leaves the context's block list and the counters of sbl_synteny_stats as they are.
 * SBL_NO_TINY_INDEX is IGNORED here: the call exists to run the small-block index.  Everything returned is copied into arrays owned
 * by the ctx, valid until the next sbl_tiny_index. */
#define SBL_TINY_INDEXED 0
#define SBL_TINY_DECLINED 1
#define SBL_TINY_NOT_ELIGIBLE 2
typedef struct { uint32_t chr, pad_; uint64_t start, end; } sbl_tiny_range;
typedef struct { uint32_t status, bif_count; uint64_t first_pos, npos, first_neg, nneg; } sbl_tiny_result;
sbl_status sbl_tiny_index(sbl_ctx *ctx, uint64_t nblocks, const uint64_t *block_first, const sbl_tiny_range *ranges, uint32_t trim_k,
                          int batched, const sbl_tiny_result **res, const sbl_inst **pos, const sbl_inst **neg);

/* TEST ENTRY POINT: the kernel that lists the touched ids for an incremental snapshot of the simplification stage, on a caller's
 * flags.  touch: nid + 1 bytes (ids 0 .. nid; id nid is never listed).  list: room for nid + 1 words -- the touched ids below nid, in any
 * order, in its first out[0] words.  out[1]: what the kernel leaves in the count word of the walking probe's list (0).  touch_after /
 * need_after: nid + 1 bytes each, what the kernel leaves in the two flag arrays (0 everywhere). */
sbl_status sbl_test_touched_list(sbl_ctx *ctx, const uint8_t *touch, uint32_t nid, uint32_t *list, uint32_t *out, uint8_t *touch_after, uint8_t *need_after);

/* TEST ENTRY POINT: the set-up of a simplification stage for (k, D) on the loaded state, one GPU -- enumeration, compact marks, instance
 * lists, positional order of the ids, block index -- and nothing after it: the state is left as it is.
 * out[0 .. 5]: ids, marks of strand 0, marks of strand 1, blocks of the block index (0: the stage keeps none), elements, 1 if the
 * index records came from the marks pass.  The arrays stay on the device until the next stage or set-up; sbl_test_graph_fetch copies the
 * first `bytes` bytes of one of them (SBL_ERR_BAD_ARG: more than it holds):
 *   0 melem[strand]   1 mid[strand]   2 maux[strand]        (uint32 per mark of the strand, ascending element)
 *   3 head[strand]    4 lsize[strand]                       (uint32 per id: first node of its list or 0xFFFFFFFF, instances)
 *   5 nnext           6 nslot          9 nidst   10 nmark   (uint32 per node: next node of the list or 0xFFFFFFFF, element slot,
 *                                                            (id << 1) | strand, index of its mark in the strand's compact arrays)
 *   7 perm                                                  (uint32 per id: the ids in positional order)
 *   8 block index                                           (4 x uint64 per block of 64 slots)
 *   11 nodeof[strand]                                       (uint32 per element slot: its node or 0xFFFFFFFF) */
sbl_status sbl_test_graph_build(sbl_ctx *ctx, uint32_t k, uint32_t D, uint32_t *out);
sbl_status sbl_test_graph_fetch(sbl_ctx *ctx, int what, int strand, void *dst, uint64_t bytes);

/* what the reference's main runs after GenerateSyntenyBlocks (src/sibelia.cpp:287-315) on the blocks of the last
 * sbl_generate_blocks: Postprocessor::GlueStripes (src/postprocessor.cpp:37-154; skipped when glue == 0) and the texts of
 * blocks_coords.txt (OutputGenerator::ListBlocksIndices, src/outputgenerator.cpp:227-233), genomes_permutations.txt
 * (ListChromosomesAsPermutations, :203-219) and coverage_report.txt (GenerateReport, :162-201), byte for byte.
 * names: record descriptions, EXACTLY sbl_nchr(ctx) pointers (NULL: those of the last sbl_load_fasta).  Host-side bookkeeping and formatting only.
 * Everything returned is owned by the ctx and valid until the next call. */
sbl_status sbl_postprocess(sbl_ctx *ctx, int glue, const char *const *names, const sbl_block **blocks, uint64_t *n,
                           const char **blocks_coords, const char **genomes_permutations, const char **coverage_report);

/* Postprocessor::GlueStripes (src/postprocessor.cpp:37-154) on a caller's block list, in place (*n updated; never grows): the
 * reference's main applies it to the blocks of every stage under -v / --allstages (src/sibelia.cpp:247-253).  Same merges in the same
 * order as the reference, found by a worklist instead of one rescan per merge (88 k instances: 0.04 s instead of a minute).
 * Host bookkeeping only: needs neither a context nor a device. */
sbl_status sbl_glue_stripes(sbl_block *blocks, uint64_t *n, uint32_t nchr);

/* OutputGenerator::ListBlocksSequences (src/outputgenerator.cpp:287-318): the text of blocks_sequences.fasta for a block list
 * (blocks == NULL: the context's current list, i.e. after sbl_generate_blocks / sbl_postprocess), spelled from the ORIGINAL
 * records kept on the device.  names as in sbl_postprocess.  Owned by the ctx, valid until the next call.
 * Per instance, in the reference's order (ONE unstable sort by |id| of a copy of the list): a header line
 *   >Seq="<description>",Strand='<+|->',Block_id=<|id|>,Start=<from>,End=<to>
 * (1-based; a reverse instance is reported from its far end, as in blocks_coords.txt), the end - start bases in lines of 80 and a
 * line feed.  Reverse instances are spelled downwards through the reference's complement table (src/dnasequence.cpp:11-28):
 * ACGT / acgt swapped, every other character -- ambiguity codes included -- unchanged.  The text is spelled by k_spell_text
 * (csrc/spell_text.hip; csrc/blockseq.hip lists its pieces) and comes back through a pinned buffer of the context, valid until the next sbl_blocks_sequences
 * or sbl_align_pairs / _unique_blocks / _groups / _block_groups or sbl_spell_text call (they share the buffer).  n == 0: empty text.  SBL_ERR_BAD_ARG: chr >= nchr,
 * end < start, end beyond the record, id == 0, no records loaded.
 * sbl_blocks_sequences_times: device time of the last call's kernel and of its device-to-host copy (event pairs). */
sbl_status sbl_blocks_sequences(sbl_ctx *ctx, const sbl_block *blocks, uint64_t n, const char *const *names,
                                const char **text, uint64_t *len);
sbl_status sbl_blocks_sequences_times(const sbl_ctx *ctx, double *kernel_ms, double *copyback_ms);

/* OutputGenerator::ListBlocksIndicesGFF (src/outputgenerator.cpp:598-631); blocks / names as above.  Host formatting only:
 * "##gff-version 2", "##source-version Sibelia 3.0.7", "##Type DNA", then per instance (one unstable sort by |id|) the tab-separated
 * columns <striped id> Sibelia synteny_block_copy <min(from, to)> <max(from, to)> . <+|-> . <|id|>.  Striped id (src/fasta.h:44-64):
 * with '|' and '.' read as blanks, a description of exactly five tokens gives its fourth; any other description stands as it is. */
sbl_status sbl_blocks_gff(sbl_ctx *ctx, const sbl_block *blocks, uint64_t n, const char *const *names,
                          const char **text, uint64_t *len);
/* OutputGenerator::ListBlocksIndices (src/outputgenerator.cpp:227-233), the blocks_coords.txt of sbl_postprocess, for any list: under
 * --allstages the reference's main writes one such file per stage (src/sibelia.cpp:300-308).  blocks / names as above. */
sbl_status sbl_blocks_coords(sbl_ctx *ctx, const sbl_block *blocks, uint64_t n, const char *const *names,
                             const char **text, uint64_t *len);

/* Postprocessor::ImproveBlockBoundaries (src/postprocessor.cpp:156-348), what the reference's main runs under --correctboundaries after
 * GlueStripes (src/sibelia.cpp:198-225, :295-298), on the context's CURRENT block list (after sbl_postprocess); chromosomes
 * 0 .. n_reference_chr - 1 are the reference set (the records of the first input file).  R = min(min_block_size, 1024)
 * (MAX_CORRECTION_RANGE, src/postprocessor.cpp:15).  The list is sorted by |id| with the reference's unstable sort (the same libstdc++
 * call on the same element order) and REPLACED: for every id with exactly one instance inside the reference set and one outside it the
 * reference instance comes first, both change sign if it lay on the negative strand, and both are re-cut (UpdateBlockBoundaries,
 * :279-293) by two local alignments -- start windows and end windows (DetermineLeft / RightProbableBoundaries :199-238,
 * GetBoundariesSequence :240-255), taken from the ORIGINAL records on the device -- run in batches by csrc/boundary_align.hip.
 * Groups are corrected in the reference's order wherever the order can matter (DESIGN.md "Boundary correction").  The three texts of
 * sbl_postprocess are rendered again; sbl_blocks_sequences / _gff / _coords with blocks == NULL then see the corrected list.
 * Where the reference is undefined: a block with start < R that has a previous block (start - R wraps as size_t, :209) is given the
 * signed result here (the window starts behind the previous block); R == 0 is SBL_ERR_BAD_ARG, as are a missing list or records and
 * n_reference_chr == 0 or >= sbl_nchr(ctx).  Windows are cut to their record.  A list is missing until sbl_generate_blocks has run; an
 * EMPTY list is a list: nothing is corrected and the texts are rendered, as the reference's loop runs over nothing (:317-348). */
sbl_status sbl_correct_boundaries(sbl_ctx *ctx, uint32_t min_block_size, uint32_t n_reference_chr, const char *const *names,
                                  const sbl_block **blocks, uint64_t *n,
                                  const char **blocks_coords, const char **genomes_permutations, const char **coverage_report);

/* The bare batched alignment behind it: Postprocessor::LocalAlignment (src/postprocessor.cpp:257-277) = SeqAn 1.3.1's
 * localAlignment(align, Score<int>(25, -75, -75)) (src/include/seqan/align/align_local_dynprog.h:229-336, :545-648, :718-751) for ndesc
 * pairs of byte strings of at most SBL_ALIGN_MAX_LEN characters each (bytes are compared as they are: N == N).
 * out_coords: 4 values per pair -- clipped begin and end position of a, then of b.  An empty string or a best score of 0: (0, na, 0, nb). */
#define SBL_ALIGN_MAX_LEN 2047
typedef struct { const uint8_t *a; const uint8_t *b; uint32_t na, nb; } sbl_align_desc;
sbl_status sbl_align_windows(sbl_ctx *ctx, uint64_t ndesc, const sbl_align_desc *descriptors, uint32_t *out_coords);

/* Counters of the last sbl_correct_boundaries (or sbl_align_windows: groups = levels = 0). */
typedef struct {
	uint64_t groups;                 /* id groups that were corrected */
	uint64_t alignments;             /* local alignments run (2 per group) */
	uint64_t levels;                 /* dependency levels: batches in which the groups were aligned */
	uint64_t launches;               /* kernel launches (a level whose trace codes exceed the cap takes several) */
	uint64_t cells;                  /* matrix cells filled */
	double kernel_ms;                /* device time of the launches (event pairs) */
} sbl_correct_stats_t;
sbl_status sbl_correct_stats(const sbl_ctx *ctx, sbl_correct_stats_t *out);

/* Base-by-base alignment of block instances (csrc/block_align.hip): what the reference's comparison tool C-Sibelia.py does with the
 * blocks of a two-genome run by handing each one to an external LAGAN process (src/csibelia/C-Sibelia.py:274-309).  LAGAN is an anchored
 * heuristic; the alignment here is defined by this project: the GLOBAL alignment of a (n bytes) and b (m bytes) with
 * match +25, mismatch -75, gap column -75 in 32-bit arithmetic, bytes compared as they are, filled from the ends
 *   S[n][m] = 0, S[i][m] = -75 (n - i), S[n][j] = -75 (m - j), S[i][j] = max(S[i+1][j+1] + (a[i] == b[j] ? 25 : -75), S[i+1][j] - 75, S[i][j+1] - 75)
 * and traced forward from (0, 0): the diagonal step if it attains the maximum, else the i step (a[i] over '-'), else the j step.
 * Only a band lo - w <= j - i <= hi + w (lo = min(0, m - n), hi = max(0, m - n)) is filled; a banded score strictly greater than
 * U(w) = 25 (min(n, m) - (w + 1)) - 75 (|m - n| + 2 (w + 1)) proves that score and trace equal the unbanded ones, otherwise w is doubled
 * and the pair runs again, until the band covers the matrix.  The first w is 64 (SBL_TEST_GALIGN_W0: test switch; results do not
 * depend on it, band_w and passes do).
 * A pair is SKIPPED -- status SBL_GALIGN_SKIPPED, no score, no runs, no rows; never an error, never a partial result -- by one of three
 * limits.  In either mode of sbl_align_set_wide (below): when the trace codes (2 bits per band cell, 4 with a gap opening cost) at the w
 * it has reached exceed the per-alignment cap (8 GiB; SBL_TEST_GALIGN_CAP_KB: test switch), and when 75 (n + m) does not fit the 32-bit
 * scores (n + m >= 2^23).  With the wide setting OFF (the default) also when the band's score diagonal no longer fits the LDS: more
 * than 12288 band offsets |m - n| + 2 w + 1, 4992 with a gap opening cost -- for pairs of bacterial blocks this is the limit that
 * binds, at the first w already once the lengths differ by more than 12159 (4863).  With the setting ON the band limit is gone and only
 * the first two remain: the cap on the codes binds, about (n + m + 1) * offsets / 8 bytes (twice that with a gap opening cost).  A
 * batch is split so that the codes of one launch stay below 32 GiB (SBL_TEST_GALIGN_TOTAL_KB: test switch).
 *
 * sbl_pair_desc: two half-open ranges of the ORIGINAL records on the device; rev: read downwards through the complement table.
 * sbl_align_run: `len` columns of one kind -- '=' equal, 'X' unequal, 'I' a[i] over '-', 'D' '-' over b[j].
 * sbl_pair_result: runs[first_run, first_run + nruns); the gapped row of a is rows[row_off, row_off + row_len), the row of b follows it
 * directly (the same length).  The rows are spelled on the device from the runs and the records and come back through the context's
 * pinned buffer.  n == 0 or m == 0 is legal: all gaps.  Everything returned is owned by the ctx and valid until the next call.
 * That pinned buffer is the ONE sbl_blocks_sequences hands its text out of: `rows` is overwritten by the next sbl_blocks_sequences as
 * well as by the next sbl_align_* call, and the text of an earlier sbl_blocks_sequences does not survive an sbl_align_* call.  A caller
 * that needs both copies the first before it asks for the second.
 * SBL_ERR_BAD_ARG: a range outside its record, end < start, a record that does not exist, no records loaded. */
#define SBL_GALIGN_OK 0
#define SBL_GALIGN_SKIPPED 1
typedef struct { uint32_t chr_a; uint64_t start_a, end_a; uint32_t rev_a; uint32_t chr_b; uint64_t start_b, end_b; uint32_t rev_b; } sbl_pair_desc;
typedef struct { uint32_t op, len; } sbl_align_run;
typedef struct { uint32_t status; int32_t score; uint32_t band_w, passes; uint64_t first_run, nruns, row_off, row_len; } sbl_pair_result;
sbl_status sbl_align_pairs(sbl_ctx *ctx, uint64_t npairs, const sbl_pair_desc *desc, const sbl_pair_result **res,
                           const sbl_align_run **runs, uint64_t *nruns, const char **rows, uint64_t *rows_len);

/* Affine gap costs for the alignment above.  `open` = o, 0 <= o <= 100000, is the cost of OPENING a gap run: a run of
 * L gap columns costs o + 75 L; match +25, mismatch -75 and the 75 per gap column stay.  An 'I' run directly followed by a 'D' run is
 * two runs.  Three matrices, filled from the ends (absent terms are minus infinity):
 *   H[n][m] = 0
 *   E[i][j] = max(E[i+1][j] - 75, H[i+1][j] - o - 75)      i < n   (a[i] over '-')
 *   F[i][j] = max(F[i][j+1] - 75, H[i][j+1] - o - 75)      j < m   ('-' over b[j])
 *   H[i][j] = max(H[i+1][j+1] + (a[i] == b[j] ? 25 : -75) [i < n, j < m], E[i][j] [i < n], F[i][j] [j < m])
 * so H[n][j] = F[n][j] = -o - 75 (m - j) and H[i][m] = E[i][m] = -o - 75 (n - i).  The trace runs from (0, 0) in state H: the diagonal
 * step if it attains H, else state E if E[i][j] attains it, else state F.  State E at (i, j) emits 'I' and then CLOSES -- back to state
 * H at (i + 1, j) -- if H[i+1][j] - o - 75 == E[i][j], otherwise it stays in E; state F likewise with 'D' along j.  The result is the
 * score H[0][0] and runs over = X I D as above; n == 0 or m == 0 scores -(o + 75 (n + m)), two empty strings 0.
 * o == 0 is the alignment above EXACTLY, ties included (E <= H everywhere, so every gap column closes), and runs the same kernel.
 * Band, certificate (the same U(w): o >= 0 only lowers a path that leaves the band) and doubling are unchanged.  With o > 0 the trace
 * codes take 4 bits per band cell -- the two caps apply to the doubled size -- and three score arrays share the 64 KiB of LDS: a pair is
 * SKIPPED beyond 4992 band offsets (12288 with o == 0), so doubling from 64 stops at w = 2048 -- unless sbl_align_set_wide (below) is on.
 * sbl_align_set_gap_open: holds for every later sbl_align_pairs / _unique_blocks / _groups / _block_groups call of the context (default 0);
 * SBL_ERR_BAD_ARG above 100000, the value stays as it was.  Not used by sbl_correct_boundaries, whose alignment is the reference's.
 * SBL_TEST_GALIGN_AFFINE=1: test switch, sends o == 0 through the three-state kernel. */
sbl_status sbl_align_set_gap_open(sbl_ctx *ctx, uint32_t open);
sbl_status sbl_align_get_gap_open(const sbl_ctx *ctx, uint32_t *open);

/* Bands beyond the LDS.  on = 1: a pair whose band has more offsets than the widest LDS class holds (12288, 4992 with a
 * gap opening cost) is no longer skipped but runs in one further band class of the same kernel, whose score arrays lie in a buffer of
 * the context on the device; nothing bounds the offsets of that class, and doubling goes on into it until the certificate holds or the
 * band covers the matrix.  The alignment's definition is untouched -- scores, ties, certificate, runs and rows of a pair do not depend
 * on the class it ran in -- only which pairs get a result changes; the per-alignment cap and n + m >= 2^23 skip as before.  on = 0
 * (the default): every call behaves as it did without the setting.
 * sbl_align_set_wide: holds for every later sbl_align_pairs / _unique_blocks / _groups / _block_groups call of the context;
 * SBL_ERR_BAD_ARG above 1, the value stays as it was.
 * sbl_align_wide_stats: what that class did in the last sbl_align_* call (all zero with the setting off); sbl_align_stats_t goes on
 * counting every class, this one included.
 * SBL_TEST_GALIGN_WIDE_FROM=<offsets>: test switch; with the setting on, pairs with more band offsets than this take the class (default
 * and most: the model's limit above; 0 sends every pair there).  Results, band_w and passes do not depend on it. */
typedef struct {
	uint64_t pairs;                  /* pairs that ran at least one pass in the class */
	uint64_t passes, launches;       /* alignments run in it; its launches */
	uint64_t cells;                  /* band slots it swept, counted as in sbl_align_stats_t */
	double kernel_ms;                /* device time of its launches (event pairs) */
} sbl_align_wide_stats_t;
sbl_status sbl_align_set_wide(sbl_ctx *ctx, uint32_t on);
sbl_status sbl_align_get_wide(const sbl_ctx *ctx, uint32_t *on);
sbl_status sbl_align_wide_stats(const sbl_ctx *ctx, sbl_align_wide_stats_t *out);

/* The pairs C-Sibelia.py aligns (determine_unique_block, src/csibelia/C-Sibelia.py:314-323) out of the context's CURRENT block list
 * (after sbl_postprocess / sbl_correct_boundaries): the ids with exactly two instances, one on records 0 .. n_reference_chr - 1 and
 * one outside them, both at least min_block_size long.  The reference instance is a; both are read on the strand the list reports.
 * Results in ascending block id, together with the ids and the descriptors that were aligned.  An empty list is a list (n = 0); a
 * missing list or records and n_reference_chr == 0 or >= sbl_nchr(ctx) are SBL_ERR_BAD_ARG. */
sbl_status sbl_align_unique_blocks(sbl_ctx *ctx, uint32_t min_block_size, uint32_t n_reference_chr, const int32_t **ids,
                                   const sbl_pair_desc **desc, uint64_t *n, const sbl_pair_result **res,
                                   const sbl_align_run **runs, uint64_t *nruns, const char **rows, uint64_t *rows_len);

/* Multiple alignment of groups of instances: centre-star on the FIRST instance of every group, defined by this
 * project -- the reference's comparison tool hands such blocks to mlagan.  A group is an ordered list of r >= 1 instances (half-open
 * ranges of the ORIGINAL records; rev: read downwards through the complement table); instance 0 is the centre c (n bases), the others
 * are members.  Every member is aligned to the centre by the banded global alignment above (a = c, b = the member; scores, tie rules,
 * band doubling, certificate and skip limits unchanged).  A 'D' run that starts at centre index p sits in SLOT p (0 <= p <= n; a pair
 * has at most one run per slot); G[p] is the longest such run over the members.  The alignment has L = n + sum G[p] columns: for
 * p = 0 .. n the G[p] columns of slot p, then (p < n) the column of centre base p.  The centre row holds '-' in slot columns; a member
 * row holds in slot p its inserted bases first and then '-' (left-justified), and in the column of centre base p its aligned base or
 * '-'.  No column is all gaps; the rows of centre and member k without the columns where both hold '-' are the two rows of
 * sbl_align_pairs for that pair.  r = 1 gives one row (L = n); n = 0 gives L = the longest member and a centre row of gaps.
 * If ANY member of a group is SKIPPED by the limits above the whole group is: status SBL_GALIGN_SKIPPED, L = 0, no rows -- never an
 * error, never a partial group, and the other groups of the call are unaffected.
 *
 * sbl_align_groups: group g is inst[group_first[g], group_first[g + 1]) (group_first: ngroups + 1 ascending offsets, the first one 0).
 * sbl_group_result: row i of the group is rows[row_off + i * L, row_off + (i + 1) * L), centre first, members in the order given.
 * sbl_member_result: one per INSTANCE, in the order of inst; a member's entry holds its pair's score, band_w and passes (score 0 in a
 * skipped group), a centre's entry is zero.  The pair passes and the gap slots are merged on the host from the runs; the rows are
 * spelled on the device (k_spell_groups) and come back through the context's pinned text buffer, under the ownership rule stated above
 * for sbl_align_pairs: everything returned is owned by the ctx, and `rows` is overwritten by the next sbl_align_* or
 * sbl_blocks_sequences call.  All offsets are 64 bit.
 * SBL_ERR_BAD_ARG: an empty group, a range outside its record, end < start, a record that does not exist, no records loaded. */
typedef struct { uint32_t chr; uint64_t start, end; uint32_t rev; } sbl_group_inst;
typedef struct { uint32_t status, ninst; uint64_t L, row_off; } sbl_group_result;
typedef struct { int32_t score; uint32_t band_w, passes; } sbl_member_result;
sbl_status sbl_align_groups(sbl_ctx *ctx, uint64_t ngroups, const uint64_t *group_first, const sbl_group_inst *inst,
                            const sbl_group_result **res, const sbl_member_result **members, const char **rows, uint64_t *rows_len);

/* The groups of the context's CURRENT block list (after sbl_postprocess / sbl_correct_boundaries): every id with at least two
 * instances of at least min_block_size bases, all of them, ordered by ascending (chr, start, end, rev) -- the first is the centre, so
 * nothing depends on an unstable sort -- and read on the strand the list reports.  Results in ascending block id, together with the
 * ids, the offsets and the descriptors that were aligned (as for sbl_align_groups).  An empty list is a list (ngroups = 0); a missing
 * list or records are SBL_ERR_BAD_ARG. */
sbl_status sbl_align_block_groups(sbl_ctx *ctx, uint32_t min_block_size, const int32_t **ids, const uint64_t **group_first,
                                  const sbl_group_inst **inst, uint64_t *ngroups, const sbl_group_result **res,
                                  const sbl_member_result **members, const char **rows, uint64_t *rows_len);

/* Counters of the last sbl_align_pairs / sbl_align_unique_blocks / sbl_align_groups / sbl_align_block_groups (there: the pairs are the
 * members, `skipped` counts skipped PAIRS, spell_ms is the time of k_spell_groups). */
typedef struct {
	uint64_t pairs, skipped;         /* pairs given; ... of which skipped */
	uint64_t passes;                 /* alignments run, band doublings included */
	uint64_t launches;               /* launches of the alignment kernel (one per band class and memory chunk of a pass) */
	uint64_t cells;                  /* band slots swept: (n + m + 1) * ceil(band offsets / 2) per pass of a pair */
	double kernel_ms, spell_ms;      /* device time of the alignment launches / of the kernel that spells the rows (event pairs) */
} sbl_align_stats_t;
sbl_status sbl_align_stats(const sbl_ctx *ctx, sbl_align_stats_t *out);

/* Variant segments of the multiple alignments (csrc/group_variants.hip): parse_alignment's rules (src/csibelia/
 * C-Sibelia.py:206-252) for the r rows of L columns of a group, on the groups of the context's LAST sbl_align_groups /
 * sbl_align_block_groups call, read from the rows that call left on the device.  A column is EQUAL if all r rows hold the same byte,
 * otherwise UNEQUAL, and then GAPPED if any row holds '-'.  The columns fall into maximal runs of equal and of unequal columns; an equal
 * run is KEPT if it starts at column 0, ends at column L or has at least 30 columns (MINIMUM_CONTEXT_SIZE); every other equal run is
 * merged into its unequal neighbours.  A SEGMENT [start, end) is a maximal stretch between kept equal runs.  Per segment: `lead` is 0 if
 * start == 0 or if the segment is one column that is not gapped (a single substitution), else 1 -- the base before the segment is
 * quoted; `before` is the number of centre-row bytes other than '-' in columns [0, start); `gapped` is 1 if any of its columns is.
 * sbl_group_segment: `group` indexes the groups of that call; the r slices rows[i][start - lead, end) -- gaps included, centre first, row
 * after row, end - start + lead bytes each -- lie at text[text_off ...].  Segments come in ascending (group, start).  Groups that were
 * skipped, groups with want[g] == 0 (want: one byte per group, NULL: all), r == 1 and L == 0 give no segments; no segments at all is a
 * result (nsegs = 0, an empty text).  Column classes, segment bounds and the slices are made by kernels; only the segments and the
 * slices come back, into buffers of their own: the `rows` of the groups call stay valid and unchanged.  Everything returned is owned by
 * the ctx until the next sbl_group_variants.
 * SBL_ERR_BAD_ARG: no groups call yet, or the last sbl_align_* call was sbl_align_pairs / sbl_align_unique_blocks (they spell their rows
 * through the same device buffers).
 * sbl_group_variants_times: device time of the last call's kernels and of the device-to-host copy of the slices (event pairs). */
typedef struct { uint64_t group, start, end, before, text_off; uint32_t lead, gapped; } sbl_group_segment;
sbl_status sbl_group_variants(sbl_ctx *ctx, const uint8_t *want, const sbl_group_segment **segs, uint64_t *nsegs,
                              const char **text, uint64_t *text_len);
sbl_status sbl_group_variants_times(const sbl_ctx *ctx, double *kernel_ms, double *copyback_ms);

/* Pairwise counts of the multiple alignments (csrc/group_distances.hip), defined by this project, on the groups of the
 * context's LAST sbl_align_groups / sbl_align_block_groups call, read from the rows that call left on the device.
 * COUNTS OF A ROW PAIR.  Rows x, y of one group (L columns, '-' is a gap) are instances i and j, i != j.  Every column is exactly one of
 *   match       both bytes are one of A C G T (exactly these four upper-case bytes) and equal
 *   mismatch    both bytes are one of A C G T and unequal
 *   ambiguous   neither byte is '-' and at least one is not one of A C G T (lower case counts here: bytes are taken as the rows hold them)
 *   gap(i->j)   x holds a byte other than '-' and y holds '-'
 *   gap(j->i)   x holds '-' and y holds a byte other than '-'
 *   (both hold '-': not counted)
 * so match + mismatch + ambiguous + gap(i->j) is the length of instance i -- if the record holds no '-' itself: a '-' in a record cannot
 * be told from a gap, as for sbl_group_variants.
 * CLASS MATRIX.  cls gives every instance of that groups call a class cls[k] < nclass, one entry per instance in the order of `inst`
 * (the pipeline: the index of the input file).  counts is M[nclass][nclass], row-major: M[f][g] is the sum, over all wanted groups that
 * were aligned, of the counts of every ORDERED pair (i, j), i != j, with cls[i] = f and cls[j] = g; its `gap` is gap(i->j).  So match,
 * mismatch and ambiguous are symmetric in (f, g), and a diagonal cell holds every unordered pair of one class twice.  Groups that were
 * skipped (SBL_GALIGN_SKIPPED), groups with want[g] == 0 (want: one byte per group, NULL: all), r == 1 and L == 0 give nothing; an
 * all-zero matrix is a result.
 * DISTANCE.  The p-distance of classes f, g is mismatch / (match + mismatch) of M[f][g]; no correction for multiple hits (no
 * Jukes-Cantor).  The alignment is centre-star: two members are compared through the columns the centre induces, not by an alignment
 * of their own.
 * The row comparisons run in a kernel and only the matrix comes back, into a buffer of its own: the `rows` of the groups call stay
 * valid and unchanged, and sbl_group_variants and sbl_group_distances may follow one groups call in either order with the same results.
 * The matrix is owned by the ctx until the next sbl_group_distances.  All sums are integers: they do not depend on the order of work.
 * SBL_ERR_BAD_ARG, checked on the host before any launch: no groups call yet, or the last sbl_align_* call was sbl_align_pairs /
 * sbl_align_unique_blocks; cls == NULL while there is at least one instance; nclass == 0 or nclass > 1024 (32 B per cell); a
 * cls[k] >= nclass.
 * sbl_group_distances_times: device time of the last call's kernel (with clearing the matrix) and of the device-to-host copy of the
 * matrix (event pairs). */
typedef struct { uint64_t match, mismatch, ambiguous, gap; } sbl_pair_counts;
sbl_status sbl_group_distances(sbl_ctx *ctx, const uint8_t *want, const uint32_t *cls, uint32_t nclass,
                               const sbl_pair_counts **counts /* nclass * nclass, row-major, owned by ctx */);
sbl_status sbl_group_distances_times(const sbl_ctx *ctx, double *kernel_ms, double *copyback_ms);

/* Concatenation of the multiple alignments (csrc/group_concat.hip), defined by this project: the rows of the groups of the
 * context's LAST sbl_align_groups / sbl_align_block_groups call, read where that call left them on the device, group after group, as one
 * FASTA record per CLASS (the pipeline: the input file) -- the core-genome alignment and its variable columns.
 * USED GROUPS.  A group is USED if want[g] != 0 (want: one byte per group, NULL: all), its status is SBL_GALIGN_OK and L > 0.  cls gives
 * every instance of that groups call a class cls[k] < nclass, one entry per instance in the order of `inst`.  A wanted, aligned group with
 * L > 0 must hold every class 0 .. nclass - 1 exactly once (so ninst == nclass): otherwise SBL_ERR_BAD_ARG, checked on the host before
 * any launch, and the message names the group.  Skipped groups, unwanted groups and groups with L == 0 give nothing and are not checked.
 * The used groups are concatenated in the order of the call; row f of the result is, group after group, the row of the instance with
 * class f.  Bytes are taken as the rows hold them, case kept.
 * MODE.  SBL_CONCAT_ALL keeps every column of every used group.  SBL_CONCAT_VARIABLE keeps a column if all nclass rows hold one of the
 * four upper-case bytes A C G T and the rows are not all equal: the columns that give at least one pair a `mismatch` in
 * sbl_group_distances' terms and no pair an `ambiguous` or a `gap`.  nclass == 1 keeps nothing.
 * TEXT.  With C the number of kept columns: for f = 0 .. nclass - 1 the bytes headers[header_first[f] .. header_first[f + 1]) as they
 * are (the caller includes '>' and the line feed), then the C kept bytes of row f in lines of `width`: a '\n' after every `width` bytes
 * and one after the last (C + ceil(C / width) bytes, the rule of blocks_sequences.fasta).  C == 0 gives the headers alone.
 * PARTS.  sbl_concat_part, one per used group in order: the group's kept columns are [first, first + ncols) of the concatenation; in
 * mode ALL ncols == L, in mode VARIABLE it may be 0.
 * SITES.  sbl_concat_site, mode VARIABLE only (mode ALL: nsites = 0), one per kept column, ascending: `col` is the column in the group,
 * `before` the number of centre-row bytes other than '-' in columns [0, col) -- the `before` of sbl_group_segment; the centre holds a
 * base in a kept column, so this is that base's index in the centre instance.
 * Column flags, their compaction, the sites and the text are made by kernels; text, parts and sites come back in buffers of their own,
 * owned by the ctx until the next sbl_group_concat: the `rows` of the groups call stay valid and unchanged, and sbl_group_variants,
 * sbl_group_distances and sbl_group_concat may follow one groups call in any order with the same results.  All offsets are 64 bit.
 * SBL_ERR_BAD_ARG, checked on the host before any launch: no groups call yet, or the last sbl_align_* call was sbl_align_pairs /
 * sbl_align_unique_blocks; width == 0; nclass == 0 or nclass > 1024; an unknown mode; cls == NULL while there is at least one instance;
 * a cls[k] >= nclass; headers == NULL or header_first == NULL; descending header offsets; a used group that breaks the class rule.
 * SBL_ERR_TOO_LARGE: a text beyond what one launch's grid covers (2^31 workgroups of 4096 bytes).
 * sbl_group_concat_times: device time of the last call's kernels and of the device-to-host copy of the text (event pairs). */
#define SBL_CONCAT_ALL 0
#define SBL_CONCAT_VARIABLE 1
typedef struct { uint64_t group, first, ncols; } sbl_concat_part;
typedef struct { uint64_t group, col, before; } sbl_concat_site;
sbl_status sbl_group_concat(sbl_ctx *ctx, const uint8_t *want, const uint32_t *cls, uint32_t nclass, uint32_t mode, uint32_t width,
                            const char *headers, const uint64_t *header_first,
                            const sbl_concat_part **parts, uint64_t *nparts, const sbl_concat_site **sites, uint64_t *nsites,
                            const char **text, uint64_t *text_len);
sbl_status sbl_group_concat_times(const sbl_ctx *ctx, double *kernel_ms, double *copyback_ms);

/* SNP-density mask of the multiple alignments (csrc/group_mask.hip), defined by this project: per member row of the groups
 * of the context's LAST sbl_align_groups / sbl_align_block_groups call, the regions in which the row differs from the centre row more
 * densely than the parameters allow, and the rows with those regions replaced by N.  Everything is bytes and integers.
 * USED GROUPS.  A group is USED if want[g] != 0 (want: one byte per group, NULL: all), its status is SBL_GALIGN_OK, L > 0 and it has at
 * least 2 rows.  There is no class argument: the reference row is the centre, row 0.
 * DIFFERENCE.  Column c of a used group is a difference of member row i >= 1 if the centre byte and the row's byte are both one of the four
 * upper-case bytes A C G T and are unequal: sbl_group_distances' `mismatch` of the pair (0, i).  The centre holds a base there, so
 * p = before(c) -- sbl_group_segment's `before`, the centre bytes other than '-' in columns [0, c) -- is unique to c among the
 * differences of the row.
 * DENSE RUN.  window W >= 1, max_diff T >= 1.  With p_0 < p_1 < ... the centre indices of the differences of ONE member row of ONE group:
 * every k with p_{k+T} - p_k < W masks the columns [col(p_k), col(p_{k+T})] of that row, inclusive -- T + 1 differences within W
 * consecutive centre bases, "more than T SNPs in a window of W".
 * INTERVAL.  The masked columns of a row are the union of those hulls, reported as maximal intervals; two hulls belong to one interval
 * only if they share a difference.  Two dense runs whose last and first differences are merely neighbours (k' = k + T + 1) are two
 * intervals and the columns between them stay.  The centre row is never masked.
 * MASKED ROWS.  The rows of the groups call with every byte other than '-' inside an interval replaced by 'N': gap bytes stay '-',
 * lower-case and ambiguous bytes become 'N', inserted columns (centre '-') inside an interval belong to it.  The rows of the groups the
 * call does not use -- unwanted, skipped, L == 0, one row -- are copied unchanged.  No difference or no interval is a result: the masked
 * rows then equal the rows.
 * sbl_mask_interval, in ascending (group, row, first), owned by the ctx until the next sbl_group_mask: `group` indexes the groups of the
 * groups call, row >= 1, [first, last] are columns of the group, inclusive, before_first / before_last their centre indices, ndiff
 * the number of differences inside (at least T + 1).
 * The masked rows go into a device buffer of the context's own with the layout of the rows (every row_off / L of sbl_group_result holds
 * for it); the `rows` of the groups call and the rows on the device stay unchanged.  The call marks the mask valid; the next
 * sbl_align_* call clears the mark.  Difference flags, their compaction, the run tests, a scan, the intervals and the masked rows are
 * made by kernels; the host reads two counts.  All offsets are 64 bit.
 * SBL_ERR_BAD_ARG, checked on the host before any launch: no groups call yet, or the last sbl_align_* call was sbl_align_pairs /
 * sbl_align_unique_blocks; window == 0; max_diff == 0.  A refused call leaves an earlier mask valid.
 * SBL_ERR_TOO_LARGE: rows beyond what one launch's grid covers.
 * sbl_group_mask_times: device time of the last call's kernels and of the device-to-host copy of the intervals (event pairs).
 * sbl_group_set_masked: with on = 1 every later sbl_group_variants, sbl_group_distances, sbl_group_concat and sbl_group_bootstrap call of the context reads
 * the masked rows instead of the rows, and is SBL_ERR_BAD_ARG while no mask is valid; with 0 (the default) they behave as without this
 * setting, byte for byte.  Anything but 0 / 1 is SBL_ERR_BAD_ARG and the value stays as it was. */
typedef struct { uint64_t group, row, first, last, before_first, before_last, ndiff; } sbl_mask_interval;
sbl_status sbl_group_mask(sbl_ctx *ctx, const uint8_t *want, uint32_t window, uint32_t max_diff,
                          const sbl_mask_interval **intervals, uint64_t *nintervals);
sbl_status sbl_group_mask_times(const sbl_ctx *ctx, double *kernel_ms, double *copyback_ms);
sbl_status sbl_group_set_masked(sbl_ctx *ctx, uint32_t on);      /* 0 (default) | 1 */
sbl_status sbl_group_get_masked(const sbl_ctx *ctx, uint32_t *on);

/* Bootstrap pair counts of the core-genome alignment (csrc/group_boot.hip), defined by this project: what a distance
 * tree of the classes (the pipeline: the input files) with bootstrap support needs from the rows of the groups of the context's LAST
 * sbl_align_groups / sbl_align_block_groups call, counted where that call left them on the device.  Everything is integers.
 * USED GROUPS.  want, cls and nclass mean what they mean for sbl_group_concat, the rule that a used group holds every class exactly once
 * included: it is checked on the host before any launch, with the same messages.
 * SITES.  The kept columns of SBL_CONCAT_VARIABLE over the used groups in call order, numbered 0 .. C - 1: every row holds one of A C G T
 * and the rows are not all equal.  *nsites = C.  *nclean = K, the columns of the used groups in which every row holds one of A C G T,
 * variable or not: the denominator of a proportion of differing sites.
 * DRAWS.  Every replicate r = 1 .. replicates makes n = draws ? draws : C draws (the pipeline passes 0).  Draw i = 0 .. n - 1 of replicate r
 * picks the site, in unsigned 64-bit arithmetic that wraps,
 *     ctr = (r << 32) | i;  z = seed + 0x9E3779B97F4A7C15 * (ctr + 1);
 *     z ^= z >> 30;  z *= 0xBF58476D1CE4E5B9;  z ^= z >> 27;  z *= 0x94D049BB133111EB;  z ^= z >> 31;
 *     site = ((z >> 32) * C) >> 32
 * a function of (seed, r, i, C) alone: no state, the same on any device and in any order of work.
 * COUNTS.  uint64 M[replicates + 1][nclass][nclass], row-major, owned by the ctx until the next sbl_group_bootstrap.  M[0][f][g]: the
 * sites in which the rows of classes f and g differ.  M[r][f][g], r >= 1: the draws of replicate r whose site has them differing (a site
 * drawn w times counts w times).  Every slab is symmetric with a zero diagonal; the values are exact for any weight a site can reach
 * (all draws on one site included).  C == 0 gives all zeros and is a result.
 * Site flags, their compaction, the packed sites (2 bits per class) and all counts are made by kernels; the replicates run in batches
 * whose count slabs fit 64 MiB of device memory, one launch and one host synchronisation per batch.  The rows stay unchanged, and this
 * call, sbl_group_variants, sbl_group_distances and sbl_group_concat may follow one groups call in any order with the same results.
 * Under sbl_group_set_masked(1) the rows are the masked rows, as for those three.
 * SBL_ERR_BAD_ARG, checked on the host before any launch: everything sbl_group_concat refuses for want / cls / nclass / the class rule and
 * the missing groups call; replicates > 100000; counts == NULL; the masked setting on without a valid mask.
 * SBL_ERR_TOO_LARGE: (replicates + 1) * nclass^2 > 2^27 cells (1 GiB of counts), refused before anything is allocated; C >= 2^32.
 * sbl_group_bootstrap_times: device time of the last call's kernels (flags, compaction, packing and counts) and of the device-to-host
 * copies of the counts (event pairs). */
sbl_status sbl_group_bootstrap(sbl_ctx *ctx, const uint8_t *want, const uint32_t *cls, uint32_t nclass, uint32_t replicates, uint64_t seed, uint32_t draws,
                               const uint64_t **counts, uint64_t *nsites, uint64_t *nclean);
sbl_status sbl_group_bootstrap_times(const sbl_ctx *ctx, double *kernel_ms, double *copyback_ms);

/* Partial groups: the soft core (csrc/sbl_groups.h, group_concat.hip, group_boot.hip), defined by this project.
 * sbl_group_set_partial: with on = 1 the class rule of every later sbl_group_concat and sbl_group_bootstrap call of the context is "a
 * used group holds every class AT MOST once": a group with fewer instances than classes is used, a group of one row included; a group
 * that holds a class twice, a class not below nclass and a group with more instances than classes are refused with the messages of the
 * strict rule.  A class that no used group holds is legal.  With 0 (the default) every entry point behaves as without this setting, byte
 * for byte.  Anything but 0 / 1 is SBL_ERR_BAD_ARG and the value stays as it was.  sbl_group_mask, sbl_group_variants and
 * sbl_group_distances take no class rule and do not look at the setting; sbl_group_set_masked combines with it freely.
 * With P the classes a used group holds:
 *   ALL        the row of a class outside P is L bytes of '-'.
 *   CLEAN      a column is clean if every row of P holds one of A C G T.
 *   VARIABLE   a column is kept (a SITE) if it is clean and the rows of P are not all equal; a group of one row has none.  In the text
 *              of SBL_CONCAT_VARIABLE the byte of a class outside P is '-'.  `before`, parts and sites are as without the setting.
 *   COUNTS     M[r][f][g] of sbl_group_bootstrap counts the draws (slab 0: the sites) whose site's group holds both f and g and in
 *              which the two differ.  *nclean is the sum of the clean columns of the used groups.  Draw rule, batches and limits stay.
 * sbl_group_bootstrap_pairs: clean[nclass][nclass] of the LAST successful sbl_group_bootstrap call, row-major, owned by the ctx until
 * the next one: clean[f][g] is the clean columns of the used groups that hold both f and g (clean[f][f]: that hold f), the denominator
 * of the pair's proportion of differing sites; symmetric.  After a call with the setting off every cell equals that call's *nclean.
 * SBL_ERR_BAD_ARG before any sbl_group_bootstrap call has succeeded, and for clean == NULL. */
sbl_status sbl_group_set_partial(sbl_ctx *ctx, uint32_t on);      /* 0 (default) | 1 */
sbl_status sbl_group_get_partial(const sbl_ctx *ctx, uint32_t *on);
sbl_status sbl_group_bootstrap_pairs(sbl_ctx *ctx, const uint64_t **clean /* nclass * nclass, row-major, owned by ctx */);

/* Neighbour joining of a batch of distance matrices (csrc/tree_nj.hip), defined by this project: the trees of the
 * replicates of a bootstrap, one workgroup per matrix, the matrix in LDS.  D holds ntrees matrices of n x n doubles, row-major, in host
 * memory.  The call needs no records and no groups call, and it reads and writes nothing the sbl_group_* calls own.
 * THE TREE of a matrix is Studier and Keppler's neighbour joining as sibelia_amd/tree.py's neighbour_joining computes it, in the same
 * float64 operations, so the lengths are the same bit for bit.  Leaves are 0 .. n - 1; join s = 0 .. n - 4 makes node n + s, the last three
 * rows hang from node 2 n - 3.  With m = n - s rows left, in the order that deleting the joined rows leaves, and a row's sum r taken over
 * those m cells (diagonal included) in this order -- m < 8: from 0.0 left to right; m >= 8: eight partial sums r[k] = a[k],
 * r[k] += a[i + k] for i = 8, 16, .. < m - m % 8, then ((r0 + r1) + (r2 + r3)) + ((r4 + r5) + (r6 + r7)), then the m % 8 tail cells left to
 * right, then 0.0 + that --
 *     Q[i][j] = ((double)(m - 2) * D[i][j] - r[i]) - r[j]; the pair is the first of the smallest Q over i < j, row-major
 *     li = dij / 2 + (r[i] - r[j]) / (double)(2 * (m - 2)), lj = dij - li; li < 0: (0, dij); else lj < 0: (dij, 0)
 *     the new row ((D[i][k] + D[j][k]) - dij) / 2 takes row and column i, D[i][i] = 0, row and column j leave
 *     the last three: ((D01 + D02) - D12) / 2, ((D01 + D12) - D02) / 2, ((D02 + D12) - D01) / 2, each x > 0 ? x : 0.0
 * with no fused multiply-add and IEEE divisions.
 * EDGES.  2 n - 3 per matrix, in the order of tree.py's Tree.edges: per join (n + s, node of row i, li), (n + s, node of row j, lj), then
 * the three edges of the last node.  SPLITS.  n - 3 per matrix (none for n == 3): splits[s] holds the leaves below node n + s as a bit
 * mask, complemented within n bits where it holds leaf 0 -- the convention of tree.py's bipartitions.
 * Both arrays are owned by the ctx until the next sbl_nj_batch.  Matrices go up and results come back in batches of 64 MiB / (8 n^2)
 * matrices, one launch and one host synchronisation per batch.  ntrees == 0 is a result: nothing is launched.
 * SBL_ERR_BAD_ARG, checked on the host before any launch: n < 3; edges or splits NULL; D NULL with ntrees > 0; a cell that is not finite;
 * a matrix that is not symmetric bit for bit; a diagonal cell that is not 0.  SBL_ERR_TOO_LARGE: n > 64 (the mask is one word).  A
 * refused call leaves the result of an earlier call valid.
 * sbl_nj_batch_times: device time of the last call's kernels and of its copies, uploads and copies back together (event pairs). */
typedef struct { uint32_t parent, child; double length; } sbl_nj_edge;
sbl_status sbl_nj_batch(sbl_ctx *ctx, const double *D /* ntrees * n * n, row-major, host */, uint32_t n, uint32_t ntrees,
                        const sbl_nj_edge **edges /* ntrees * (2n - 3) */, const uint64_t **splits /* ntrees * (n - 3) */);
sbl_status sbl_nj_batch_times(const sbl_ctx *ctx, double *kernel_ms, double *copy_ms /* upload + copy-back */);

/* Fitch parsimony of the sites on a tree (csrc/group_parsimony.hip), defined by this project: which site changes on
 * which branch.  The SITES 0 .. C - 1 are those of the context's LAST successful sbl_group_bootstrap call, read where that call left
 * them packed on the device (2 bits per class, presence words under sbl_group_set_partial); its nclass, C and partial setting are taken
 * from the context.  sbl_group_concat, sbl_group_variants, sbl_group_distances, sbl_group_mask and sbl_nj_batch may run in between
 * without changing the result.  Everything is integers.
 * THE TREE.  Unrooted and binary over leaves 0 .. n - 1 (the classes) and internal nodes n .. 2 n - 3, given as 2 n - 3 edges; an edge's
 * two nodes may stand in either order and its length is ignored.  It is read from leaf 0: `top` is the internal node next to leaf 0,
 * every node but leaf 0 has a parent, parent(top) is leaf 0, every internal node has two children.
 * SETS.  The code of a base is (ch >> 1) & 3: A = 0, C = 1, T = 2, G = 3.  A present leaf's set is 1 << code; under the partial setting a
 * leaf whose class the site's group does not hold has the set 0xF.
 * BOTTOM-UP.  Internal v with children a, b: S(v) = S(a) & S(b) if that is not 0, else S(a) | S(b) and the site takes one step.  Then,
 * with R = S(leaf 0), the site takes one more step if R & S(top) == 0.
 * TOP-DOWN.  The state of leaf 0 is its base; of an absent leaf 0, the lowest code in S(top).  Every other node takes its parent's state
 * if S(v) holds it, else the lowest code in S(v): an absent leaf takes its parent's state and carries no change.
 * CHANGES.  One lies on the edge (parent(v), v) at a site iff the two states differ; from is the parent's state -- the side of leaf 0 --
 * and to the child's.  A site has as many changes as steps.  changes: all of them in ascending (site, edge), edge the index into the
 * caller's edges.  edge_counts[edge][from * 4 + to]: the changes of the edge by kind, the diagonal 0.  steps[site]; minsteps[site]: the
 * distinct bases among the site's present leaves minus 1 (none present: 0); a site with steps > minsteps is homoplasic.
 * One lane per site: k_fitch_steps (sets in LDS, steps and minsteps), an exclusive scan of the steps to the offsets of the sites'
 * records, k_fitch_changes (bottom-up again, top-down, the records and a histogram per workgroup, flushed with 64-bit integer adds).
 * All four arrays are owned by the ctx until the next successful sbl_group_parsimony.  C == 0 is a result: nothing is launched, steps,
 * minsteps and changes are empty and the counts 0.  A refused call leaves the result of an earlier call valid.
 * SBL_ERR_BAD_ARG, checked on the host before any launch: no successful sbl_group_bootstrap call; n is not that call's nclass; n < 3; an
 * out pointer or edges is NULL; an edge names a node >= 2 n - 2; the edges are not a tree in which every leaf has degree 1 and every
 * internal node degree 3.  SBL_ERR_TOO_LARGE: n > 64 (the limit of sbl_nj_batch and of 64-bit file masks), before any launch; a change
 * list above 1 GiB (2^26 changes), known after the first pass and the scan.
 * sbl_group_parsimony_times: device time of the last call's two passes and scan and of the device-to-host copies (event pairs). */
typedef struct { uint64_t site; uint32_t edge; uint8_t from, to, pad_[2]; } sbl_parsimony_change;
sbl_status sbl_group_parsimony(sbl_ctx *ctx, const sbl_nj_edge *edges /* 2n - 3 */, uint32_t n,
                               const uint64_t **edge_counts /* (2n - 3) * 16 */, const uint8_t **steps /* C */, const uint8_t **minsteps /* C */,
                               const sbl_parsimony_change **changes, uint64_t *nchanges);
sbl_status sbl_group_parsimony_times(const sbl_ctx *ctx, double *kernel_ms, double *copyback_ms);

/* The calls C-Sibelia.py makes from the regions no block covers (src/csibelia/C-Sibelia.py:325-338, :373-427), by
 * interval bookkeeping on the host (csrc/uncovered.hip).  `blocks` holds nlists block lists one after the other -- list l is
 * blocks[list_first[l], list_first[l + 1]) (nlists + 1 ascending offsets, the first one 0) -- the lists of the stages in order, the LAST
 * one the final list; records 0 .. n_reference_chr - 1 are the reference set.  Ranges are 0-based and half-open.
 * A block is MIXED in a list if it has an instance on a reference record and one off them.  A base is COVERED if an instance of a
 * mixed block of ANY list holds it.  main(x) is the largest |id| among the mixed blocks of the FINAL list with an instance that holds
 * base x, 0 if there is none.  For every maximal uncovered run [start, end) of a record with end - start > min_block_size, in record
 * order and ascending start, one call:
 *   SBL_CALL_DELETION   the run lies on a reference record: ref_chr = chr, pos = start
 *   SBL_CALL_INSERTION  the run lies on another record, start > 0, block b = main(start - 1) != 0 has exactly two instances in the final
 *                       list, one in each set, both at least min_block_size long (the rule of sbl_align_unique_blocks), and
 *                       pos = (both on the same strand ? end : start) of its reference instance is > 0: ref_chr = that instance's record
 *   SBL_CALL_UNMAPPED   any other run off the reference records: ref_chr = 0, pos = 0
 * Owned by the ctx, valid until the next sbl_uncovered_calls.  SBL_ERR_BAD_ARG: no records loaded, nlists == 0, offsets that do not
 * start at 0 or descend, n_reference_chr == 0 or >= sbl_nchr(ctx), and what sbl_blocks_sequences refuses in a list. */
#define SBL_CALL_DELETION 0
#define SBL_CALL_INSERTION 1
#define SBL_CALL_UNMAPPED 2
typedef struct { uint32_t kind, chr; uint64_t start, end; uint32_t ref_chr, pad_; uint64_t pos; } sbl_uncovered_call;
sbl_status sbl_uncovered_calls(sbl_ctx *ctx, uint64_t nlists, const uint64_t *list_first, const sbl_block *blocks, uint32_t min_block_size,
                               uint32_t n_reference_chr, const sbl_uncovered_call **calls, uint64_t *ncalls);

/* Text put together on the device from the ORIGINAL records (csrc/spell_text.hip, k_spell_text): the concatenation of npieces pieces in
 * the order given.  A piece is
 *   SBL_PIECE_LITERAL  bytes [start, end) of `literals` (literal_len bytes), as they are; chr ignored, width 0
 *   SBL_PIECE_RECORD   bases [start, end) of record chr, forward, upper-cased ('a' .. 'z' only); width > 0: in lines -- a line feed
 *                      after every `width` bases and one after the last base (none for an empty range)
 * All offsets are 64 bit.  The text comes back through the context's pinned text buffer under the ownership rule stated for
 * sbl_align_pairs: it is overwritten by the next sbl_spell_text, sbl_blocks_sequences or sbl_align_* call.  npieces == 0: empty text.
 * Every argument is checked on the host before anything is launched.  SBL_ERR_BAD_ARG: no records loaded, an unknown kind, a record
 * that does not exist, end < start, a range beyond its record or beyond the literal text, a wrapped literal.
 * sbl_spell_text_times: device time of the last call's kernel and of its device-to-host copy (event pairs). */
#define SBL_PIECE_LITERAL 0
#define SBL_PIECE_RECORD 1
typedef struct { uint32_t kind, chr; uint64_t start, end; uint32_t width, pad_; } sbl_text_piece;
sbl_status sbl_spell_text(sbl_ctx *ctx, uint64_t npieces, const sbl_text_piece *pieces, const char *literals, uint64_t literal_len,
                          const char **text, uint64_t *text_len);
sbl_status sbl_spell_text_times(const sbl_ctx *ctx, double *kernel_ms, double *copyback_ms);

/* Replaces BlockFinder::SerializeGraph (src/serialization.cpp:112-138; defined for records of at least k + 1 characters -- the
 * reference walks off the end of a shorter one): DOT text of the UNcondensed de Bruijn graph of the
 * current state, one line per (k+1)-window, generated on the device (a debugging dump: main only reaches it with -q and never
 * with production options).  Owned by the ctx, valid until the next call. */
sbl_status sbl_serialize_graph(sbl_ctx *ctx, uint32_t k, const char **text, uint64_t *len);

/* H0: the k-mer hash of the reference's hashing.h (SlidingWindow / KMerHashFunction, src/hashing.h:14-112; HASH_BASE 57,
 * arithmetic mod 2^64) for every k-mer of the current state: strand 0 then strand 1 (complemented characters, walk order),
 * chromosomes ascending.  The reference's production path never executes it; provided with a known-answer test.
 * Array owned by the ctx, valid until the next call. */
sbl_status sbl_kmer_hashes(sbl_ctx *ctx, uint32_t k, const uint64_t **values, uint64_t *n);

/* The reference's rand() is process-global: besides sanitising ambiguous bases (src/indexedsequence.cpp:31-37) it names the two
 * temporary files every index built WITHOUT -r spills its suffix array to (src/platform.cpp:52-58 via src/vertexenumeration.cpp:101,125:
 * 24 draws per index).  A context owns its stream; sbl_set_tempfile_mode(ctx, 1) makes every full-state index (sbl_simplify_stage,
 * sbl_list_edges, sbl_generate_blocks' main index, sbl_enumerate) draw those 24 values after its sanitising draws, as
 * BlockFinder(chrList, tempDir) does -- nothing is spilled, only the stream stays in step.  sbl_rand_advance skips n values, for a
 * host whose surrounding code consumes the same stream in other places. */
sbl_status sbl_set_tempfile_mode(sbl_ctx *ctx, int on);
sbl_status sbl_rand_advance(sbl_ctx *ctx, uint64_t n);

/* Stage-boundary checkpoint of the resident state (sequences + original positions), device to device.
 * The reference keeps no resumable state; the stage boundary is the natural one. */
sbl_status sbl_save_state(sbl_ctx *ctx);
sbl_status sbl_restore_state(sbl_ctx *ctx);

sbl_status sbl_last_stats(const sbl_ctx *ctx, sbl_stage_stats *out);
const char *sbl_last_error(const sbl_ctx *ctx);
const char *sbl_strerror(sbl_status s);

/* ---- Multi-GPU (one context per GPU).  The reference is a single-threaded CPU program with no
 * counterpart; these entry points attach a communicator to a context, after which the enumeration inside
 * sbl_enumerate / sbl_simplify_stage / sbl_list_edges shards the k-mer table by hash prefix (k <= 32; k > 32: see sbl_longk_* below):
 * every GPU turns its contiguous slice of base positions into 16-B k-mer records (one per position, no local
 * pre-aggregation), partitions them by hash prefix and sends every owner GPU its contiguous bucket range in ONE
 * all-to-all; owners classify their buckets (LDS tables), the bifurcation codes and the member marks are all-gathered.  Simplification is globally ordered and runs replicated (bit-identical) on
 * every attached GPU.  The calls are collective: every attached context must make them with the same arguments.
 *   RCCL transport (one process or thread per GPU, xGMI): rank 0 calls sbl_comm_unique_id, the host distributes the
 *   128 bytes (MPI, torch.distributed, a file), every rank calls sbl_comm_attach_rccl.
 *   Local transport: contexts of ONE process driven by one host thread each (device-to-device copies);
 *   used by the tests to run several virtual ranks on a single GPU. */
#define SBL_COMM_ID_BYTES 128
typedef struct sbl_group sbl_group;
sbl_status sbl_comm_unique_id(void *id /* SBL_COMM_ID_BYTES */);
sbl_status sbl_comm_attach_rccl(sbl_ctx *ctx, uint32_t rank, uint32_t nranks, const void *id);
sbl_group *sbl_group_create_local(uint32_t nranks);
void sbl_group_destroy(sbl_group *group);
sbl_status sbl_comm_attach_local(sbl_ctx *ctx, sbl_group *group, uint32_t rank);
sbl_status sbl_comm_detach(sbl_ctx *ctx);

/* The layout arithmetic of the sharded table, device-free (what the pipeline itself uses; for tests and for a host that wants to
 * size its buffers): tiles scanned by `rank`, first bucket of every owner (owner(b) = (b * nranks) >> bits), and -- given the
 * all-gathered count matrix count[p * nranks + q] = records p holds for owner q, and where the owners' ranges start in this
 * rank's partitioned arrays -- the byte counts / offsets of the one all-to-all. */
sbl_status sbl_shard_layout(uint32_t nranks, uint32_t rank, uint32_t bits, uint64_t ntiles, uint32_t *first_bucket /* nranks + 1 */, uint64_t *tile_range /* 2 */);
sbl_status sbl_shard_exchange_plan(uint32_t nranks, uint32_t rank, const uint64_t *count, const uint32_t *send_at /* nranks + 1 */, uint64_t record_bytes,
                                   uint64_t *sbytes, uint64_t *soff, uint64_t *rbytes, uint64_t *roff, uint64_t *nrecv);

/* k > 32 with a communicator attached: the exact rank doubling of ONE job is split over the GPUs (csrc/longk.hip, "sharded rank
 * doubling"; replaces the single-threaded suffix array of EnumerateBifurcationsSArrayInRAM, src/vertexenumeration.cpp:263-364, for
 * BASELINE.json's config 5).  Two partitions of the suffixes of the superGenome S (np = 2E - 1 + k positions) and one exchange
 * between them per doubling round: the POSITION side (rank r owns S[first[r], first[r + 1]) and a halo of H ranks behind it) and the
 * SORTED side (rank q owns an interval of the global sorted order; owner = binary search in its bounds).  The layout arithmetic,
 * device-free, as the pipeline itself calls it:
 *   sbl_longk_slices        first[r] = np * r / nranks
 *   sbl_longk_value_bounds  equal parts of the value range [0, maxvalue] (round 1 routes by the base-5 value of 8 symbols)
 *   sbl_longk_owner         largest q < nranks with bounds[q] <= x (position owner: bounds = first; sorted-side owner: bounds = G)
 *   sbl_longk_halo_plan     byte counts / offsets (4-B ranks) of the halo fetch: what `rank` sends to every peer out of its slice,
 *                           what it receives from every peer into its halo of H positions. */
sbl_status sbl_longk_slices(uint32_t nranks, uint64_t np, uint64_t *first /* nranks + 1 */);
sbl_status sbl_longk_value_bounds(uint32_t nranks, uint64_t maxvalue, uint64_t *bounds /* nranks + 1 */);
sbl_status sbl_longk_owner(uint32_t nranks, const uint64_t *bounds /* nranks + 1 */, uint64_t x, uint32_t *owner);
sbl_status sbl_longk_halo_plan(uint32_t nranks, uint32_t rank, uint64_t np, uint64_t H, uint64_t *sbytes, uint64_t *soff, uint64_t *rbytes, uint64_t *roff);

/* Tuning knob (0 = default): number of bifurcation ids speculatively committed per ordered round. */
sbl_status sbl_set_window(sbl_ctx *ctx, uint32_t window);

#ifdef __cplusplus
}
#endif
#endif
