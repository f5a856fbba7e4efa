"""Canonical byte serialisations of hot-path results (shared by tests, bench and smoke).

These are the exact layouts the golden-vector generator writes (tests/golden/gen/ref_dump.cpp),
so that sha256(serialise(result)) can be compared with tests/golden/vectors.json:

  enum   u32 bif_count | for strand in (+,-): u64 n, n x (u32 id, u32 chr, u32 pos) in (chr,pos) order
  state  u64 bulges | u32 nchr | per chr: u64 len, len bytes, len x u32 original positions
  dot    text of BlockFinder::SerializeCondensedGraph (reference src/serialization.cpp:88-110)
  blocks u64 n | n x (i32 signed block id, u32 chr, u64 start, u64 end): BlockFinder::GenerateSyntenyBlocks' result, in its order
  write  blocks (as above, after GlueStripes) | 3 x (u64 len, text): blocks_coords.txt, genomes_permutations.txt, coverage_report.txt
  hash   for strand in (+,-), per chromosome: u64 n, n x u64 k-mer hashes of the reference's hashing.h in walk order
"""
from __future__ import annotations

import hashlib
import struct
from typing import List, Sequence, Tuple

import numpy as np


def enum_bytes(bif_count: int, pos: np.ndarray, neg: np.ndarray) -> bytes:
    """pos/neg: uint32 arrays of shape (n, 3) with columns (id, chr, pos)."""
    out = [struct.pack("<I", bif_count)]
    for a in (pos, neg):
        a = np.ascontiguousarray(a, dtype="<u4").reshape(-1, 3)
        out.append(struct.pack("<Q", a.shape[0]))
        out.append(a.tobytes())
    return b"".join(out)


def state_bytes(bulges: int, seqs: Sequence[bytes], opos: Sequence[np.ndarray]) -> bytes:
    out = [struct.pack("<QI", bulges, len(seqs))]
    for s, p in zip(seqs, opos):
        out.append(struct.pack("<Q", len(s)))
        out.append(bytes(s))
        out.append(np.ascontiguousarray(p, dtype="<u4").tobytes())
    return b"".join(out)


BLOCK_DTYPE = np.dtype([("id", "<i4"), ("chr", "<u4"), ("start", "<u8"), ("end", "<u8")])


def blocks_bytes(blocks: np.ndarray) -> bytes:
    b = np.ascontiguousarray(blocks, dtype=BLOCK_DTYPE)
    return struct.pack("<Q", len(b)) + b.tobytes()


def hash_bytes(values: np.ndarray, lens: Sequence[int], k: int) -> bytes:
    """values: flat uint64 array, strand 0 then strand 1, chromosomes ascending; lens: chromosome lengths."""
    values = np.ascontiguousarray(values, dtype="<u8")
    out, at = [], 0
    for _ in range(2):
        for n in lens:
            m = n - k + 1 if n >= k else 0
            out.append(struct.pack("<Q", m))
            out.append(values[at:at + m].tobytes())
            at += m
    assert at == len(values)
    return b"".join(out)


EDGE_DTYPE = np.dtype([("chr", "<u4"), ("strand", "<u4"), ("start_vertex", "<u4"), ("end_vertex", "<u4"),
                       ("pos", "<u4"), ("len", "<u4"), ("orig_pos", "<u4"), ("orig_len", "<u4"),
                       ("first_char", "S1"), ("_pad", "V3")])


def dot_text(edges: np.ndarray) -> bytes:
    """Edge records (EDGE_DTYPE) -> the reference's DOT text (src/serialization.cpp:92-109)."""
    lines = ["digraph G", "{", "rankdir=LR"]
    for e in edges:
        lines.append('%d -> %d [color="%s", label="chr=%d pos=%d len=%d orpos=%d orlen=%d  ch=\'%s\'"];' % (
            e["start_vertex"], e["end_vertex"], "blue" if e["strand"] == 0 else "red",
            np.int32(e["chr"]), np.int32(e["pos"]), np.int32(e["len"]), np.int32(e["orig_pos"]), np.int32(e["orig_len"]),
            e["first_char"].decode("latin1")))
    lines.append("}")
    return ("\n".join(lines) + "\n").encode("latin1")


def sha256(b: bytes) -> str:
    return hashlib.sha256(b).hexdigest()


# ------------------------------------------------------------------------------------------ alignments of unique blocks (--maf, --variants)

MINIMUM_CONTEXT_SIZE = 30                         # src/csibelia/C-Sibelia.py:20
# reverse_complementary (C-Sibelia.py:84-90) maps upper-case ACGT; both loaders upper-case the records, so that is all a run ever sees.
# The table also maps acgt, as the device's complement table (csrc/sbl_dna.h) does: rows of a '-' instance and alleles never disagree.
_COMPLEMENT = bytes.maketrans(b"ACGTacgt", b"TGCAtgca")


def strip_chr_id(chr_id: str) -> str:
    """strip_chr_id (C-Sibelia.py:92-96): gi|...|ref|NC_000000.1| -> NC_000000."""
    part = chr_id.split("|")
    return part[-2].split(".")[0] if len(part) == 5 else chr_id


def maf_line(name: str, start: int, end: int, reverse: bool, record_size: int, row: bytes) -> bytes:
    """One `s` line of write_alignments_maf (C-Sibelia.py:473-484) for the instance [start, end) (0-based, half-open) of a record:
    s <description> <start> <size> <strand> <record size> <row>; start is 0-based and counted from the record's end for '-'."""
    at = record_size - end if reverse else start
    return b"s %s %d %d %s %d %s" % (name.encode(), at, end - start, b"-" if reverse else b"+", record_size, row)


def maf_text(groups, gap_open: int = 0) -> bytes:
    """write_alignments_maf: `##maf version=1`, an empty line, then per group `a`, its `s` lines (maf_line) and an empty line.
    gap_open > 0 (--gapopen) is recorded in a comment line `# gapopen=N` after the first."""
    out = [b"##maf version=1\n" if not gap_open else b"##maf version=1\n# gapopen=%d\n" % gap_open]
    for lines in groups:
        out.append(b"a")
        out += list(lines)
        out.append(b"")
    return b"\n".join(out) + b"\n"


def variants_from_runs(runs, row_a: bytes, row_b: bytes, start: int, end: int, reverse: bool):
    """parse_alignment (C-Sibelia.py:206-252) from the runs of an alignment -- (op, length) with op in '=XID', '=' the only kind whose
    columns are equal -- instead of a scan of the rows.  [start, end): the reference-side instance, 0-based half-open; reverse: it is
    read on '-'.  -> [(POS, REF, ALT)].
      * maximal stretches of equal / unequal columns become segments;
      * an equal segment shorter than 30 columns that is not the first is merged into the unequal segments around it;
      * each unequal segment is one variant;
      * POS comes from the reference-side map of columns to 1-based positions -- start + 1 upwards, or `end` downwards for a '-'
        instance, advancing on every column whose reference row is no gap;
      * the base before the segment is included (shift = 1: POS - 1, one more column) unless the segment starts the alignment or is a
        single substitution;
      * alleles are the rows' columns without gaps, reverse-complemented when the reference instance is on '-' (an empty one stays
        empty here; vcf_text writes '.')."""
    stretches = []                                  # [first column, one past the last, equal?, reference bases before it]
    col = used = 0
    for op, length in runs:
        op = chr(op) if isinstance(op, int) else op
        if not length:
            continue
        if stretches and stretches[-1][2] == (op == "="):
            stretches[-1][1] += length
        else:
            stretches.append([col, col + length, op == "=", used])
        col += length
        used += length if op != "D" else 0
    if not stretches:
        return []
    before = {s[0]: s[3] for s in stretches}
    segment, at = [], 0
    for prev, now in zip(stretches, stretches[1:]):
        if not prev[2] or now[0] - at >= MINIMUM_CONTEXT_SIZE or at == 0:
            segment.append([at, now[0], prev[2]])
            at = now[0]
        elif segment:
            at = segment.pop()[0]
    segment.append([at, col, stretches[-1][2]])
    first, step = (end, -1) if reverse else (start + 1, 1)
    out = []
    for s, e, equal in segment:
        if equal:
            continue
        snp = e - s == 1 and row_a[s:e] != b"-" and row_b[s:e] != b"-"
        shift = 0 if s == 0 or snp else 1
        ref, alt = row_a[s - shift:e].replace(b"-", b""), row_b[s - shift:e].replace(b"-", b"")
        if reverse:
            ref, alt = ref.translate(_COMPLEMENT)[::-1], alt.translate(_COMPLEMENT)[::-1]
        out.append((first + step * before[s] - shift, ref, alt))
    return out


def vcf_text(reference_name: str, records, gap_open: int = 0) -> bytes:
    """write_vcf_header (C-Sibelia.py:433-440) with ##source=sibelia_amd, then Variant.get_vcf_record (:177-180) per record
    (reference record description, POS, REF, ALT), sorted by (description, POS) as variant_key does (:502-503): eight tab-separated
    columns, '.' for an empty allele."""
    out = vcf_header_lines(reference_name, gap_open)
    for name, pos, ref, alt in sorted(records, key=lambda r: (r[0], r[1])):
        out.append("\t".join([strip_chr_id(name), str(pos), ".", ref.decode("latin1") or ".", alt.decode("latin1") or ".", ".", ".", "."]))
    return ("\n".join(out) + "\n").encode("latin1")


def vcf_header_lines(reference_name: str, gap_open: int = 0):
    """gap_open > 0 (--gapopen) is recorded in a line `##sibelia_amd_gapopen=N` after `##source`."""
    return ["##fileformat=VCFv4.1", "##source=sibelia_amd"] + (["##sibelia_amd_gapopen=%d" % gap_open] if gap_open else []) + ["##reference=" + strip_chr_id(reference_name),
            '##INFO=<ID=SVTYPE,Number=1,Type=String,Description="Type of structural variant">',
            '##INFO=<ID=IMPRECISE,Number=0,Type=Flag,Description="Imprecise structural variation">',
            '##INFO=<ID=CIPOS,Number=2,Type=Integer,Description="Confidence interval around POS for imprecise variants">',
            "\t".join(["#CHROM", "POS", "ID", "REF", "ALT", "QUAL", "FILTER", "INFO"])]


# ------------------------------------------------------------------------------------------ calls from the multiple alignments (--multivariants)

def group_variants_records(segments, start: int, end: int, reverse: bool):
    """The calls of ONE aligned group from its segments as BlockFinder.group_variants returns them -- (group, first
    column, one past the last, centre bases before it, lead, [gapped slice per row, centre first]) -- and the centre's instance
    [start, end) (0-based, half-open; reverse: read on '-').  -> [(POS, [allele per row])]: POS and alleles exactly as
    variants_from_runs makes them for two rows -- lead is its shift, the alleles are the slices without gaps, reverse-complemented
    for a centre on '-'."""
    first, step = (end, -1) if reverse else (start + 1, 1)
    out = []
    for _, _s, _e, before, lead, slices in segments:
        alleles = [x.replace(b"-", b"") for x in slices]
        if reverse:
            alleles = [x.translate(_COMPLEMENT)[::-1] for x in alleles]
        out.append((first + step * before - lead, alleles))
    return out


FORMAT_GT_LINE = '##FORMAT=<ID=GT,Number=1,Type=String,Description="Genotype">'


def multi_vcf_text(reference_name: str, sample_names: Sequence[str], records, gap_open: int = 0) -> bytes:
    """A multi-sample VCF: the header of vcf_text with the FORMAT line of GT before the column line, which gets FORMAT and one column
    per sample.  records: (description of the centre's record, POS, block id, REF allele, [allele per sample, None where the sample has
    no instance in the block]), sorted here by (description, POS, block id).  ALT holds the distinct alleles other than REF in order of
    first appearance over the samples; an empty allele is written '.'; a sample holds the index of its allele (0 REF, 1 .. ALT) or '.'."""
    head = vcf_header_lines(reference_name, gap_open)
    out = head[:-1] + [FORMAT_GT_LINE, head[-1] + "\t" + "\t".join(["FORMAT"] + list(sample_names))]
    for name, pos, _block, ref, alleles in sorted(records, key=lambda r: (r[0], r[1], r[2])):
        seen = [ref]
        for x in alleles:
            if x is not None and x not in seen:
                seen.append(x)
        alt = ",".join(x.decode("latin1") or "." for x in seen[1:]) or "."
        gt = ["." if x is None else str(seen.index(x)) for x in alleles]
        out.append("\t".join([strip_chr_id(name), str(pos), ".", ref.decode("latin1") or ".", alt, ".", ".", ".", "GT"] + gt))
    return ("\n".join(out) + "\n").encode("latin1")


DISTANCE_COUNTS_COLUMNS = ("file_a", "file_b", "blocks", "match", "mismatch", "ambiguous", "gap_a", "gap_b")


def distance_counts_text(names: Sequence[str], counts, blocks, gap_open: int = 0) -> bytes:
    """The file of --distancecounts: tab-separated, a line of column names, then one line per pair of files a < b in
    input order.  counts[a][b] = (match, mismatch, ambiguous, gap(a -> b)) as BlockFinder.group_distances returns them; blocks[a][b]:
    the used and aligned blocks with an instance in both.  gap_a = counts[a][b] gap, the bases of a opposite a gap of b; gap_b =
    counts[b][a] gap.  gap_open > 0 (--gapopen) is recorded in a line `# gapopen=N` before the column names."""
    out = (["# gapopen=%d" % gap_open] if gap_open else []) + ["\t".join(DISTANCE_COUNTS_COLUMNS)]
    for a in range(len(names)):
        for b in range(a + 1, len(names)):
            match, mismatch, ambiguous, gap_a = (int(x) for x in counts[a][b])
            out.append("\t".join([names[a], names[b]] + [str(x) for x in (int(blocks[a][b]), match, mismatch, ambiguous, gap_a, int(counts[b][a][3]))]))
    return ("\n".join(out) + "\n").encode("latin1")


def p_distance_text(match: int, mismatch: int) -> str:
    """mismatch / (match + mismatch) to six decimals, made from the integers alone -- (mismatch 10^6 + c / 2) / c with c = match +
    mismatch, a tie going up -- so that the text is the same on every host; `nan` for c = 0."""
    c = int(match) + int(mismatch)
    if c == 0:
        return "nan"
    v = (int(mismatch) * 10 ** 6 + c // 2) // c
    return "%d.%06d" % (v // 10 ** 6, v % 10 ** 6)


def distances_text(names: Sequence[str], counts, complain=None) -> bytes:
    """The file of --distances: a square matrix in PHYLIP format -- the number of files, then per file its name and
    one value per file, separated by single blanks; 0.000000 on the diagonal, p_distance_text of counts[a][b] elsewhere.  A pair
    without a column that holds A C G T on both sides is written `nan` and named through `complain`, one line per pair a < b."""
    out = [str(len(names))]
    for a in range(len(names)):
        row = [names[a]]
        for b in range(len(names)):
            v = "0.000000" if a == b else p_distance_text(counts[a][b][0], counts[a][b][1])
            if v == "nan" and a < b and complain is not None:
                complain("no distance between %s and %s: the blocks used hold no column with one of A C G T in both\n" % (names[a], names[b]))
            row.append(v)
        out.append(" ".join(row))
    return ("\n".join(out) + "\n").encode("latin1")


CORE_PARTITIONS_COLUMNS = ("block", "first", "last")
CORE_SITES_COLUMNS = ("column", "block", "record", "position", "strand")
CORE_WIDTH = 80                                   # bases per line of --corealignment / --coresnps


def core_headers(names: Sequence[str]) -> Tuple[bytes, List[int]]:
    """The FASTA headers of --corealignment / --coresnps as BlockFinder.group_concat takes them: `>` + the file's base name + a line
    feed per input file, in one blob, and their len(names) + 1 offsets."""
    blob, first = bytearray(), [0]
    for n in names:
        blob += b">" + n.encode("latin1") + b"\n"
        first.append(len(blob))
    return bytes(blob), first


def _core_comments(gap_open: int, coremin: int) -> List[str]:
    """the comment lines of the --core files: `# gapopen=N` for gap_open > 0 (--gapopen), then `# coremin=M` for coremin > 0 (--coremin
    below the number of files: the soft core)"""
    return (["# gapopen=%d" % gap_open] if gap_open else []) + (["# coremin=%d" % coremin] if coremin else [])


def core_partitions_text(rows: Sequence[Tuple[int, int, int]], gap_open: int = 0, coremin: int = 0) -> bytes:
    """The file of --corepartitions: tab-separated, a line of column names, then one line per used block in ascending
    id.  rows: (block id, first column, number of columns) with the first column counted from 0 as BlockFinder.group_concat returns the
    parts; written 1-based and inclusive.  gap_open > 0 (--gapopen) is recorded in a line `# gapopen=N` before the column names, coremin > 0
    in a line `# coremin=M` after it."""
    out = _core_comments(gap_open, coremin) + ["\t".join(CORE_PARTITIONS_COLUMNS)]
    out += ["%d\t%d\t%d" % (block, first + 1, first + ncols) for block, first, ncols in rows]
    return ("\n".join(out) + "\n").encode("latin1")


def core_sites_text(rows: Sequence[Tuple[int, str, int, int, bool, int]], gap_open: int = 0, coremin: int = 0) -> bytes:
    """The file of --coresites: tab-separated, a line of column names, then one line per column of --coresnps, numbered
    from 1.  rows: (block id, record name, start, end, rev, before) -- the centre instance of the block (0-based, half-open, on the
    first file) and the index of the column's base in it; the position is 1-based on the record: start + before + 1 for a forward
    instance, end - before for a reverse one.  gap_open > 0 and coremin > 0 are recorded as for core_partitions_text."""
    out = _core_comments(gap_open, coremin) + ["\t".join(CORE_SITES_COLUMNS)]
    for i, (block, record, start, end, rev, before) in enumerate(rows):
        out.append("%d\t%d\t%s\t%d\t%s" % (i + 1, block, record, end - before if rev else start + before + 1, "-" if rev else "+"))
    return ("\n".join(out) + "\n").encode("latin1")


CORE_BRANCHES_COLUMNS = ("branch", "files", "length", "support", "changes", "transitions", "transversions")
CORE_BRANCH_SITES_COLUMNS = CORE_SITES_COLUMNS + ("branch", "from", "to", "steps", "minsteps")
PARSIMONY_BASES = "ACTG"                          # the base of a code (ch >> 1) & 3
PARSIMONY_TRANSITIONS = ((0, 3), (3, 0), (1, 2), (2, 1))      # A <-> G, C <-> T as (from, to)


def parsimony_summary(steps, minsteps) -> str:
    """the line `# sites=C steps=S minsteps=M homoplasic=H ci=X` of --corebranches / --corebranchsites: the sums over the sites, the
    sites with more steps than their bases need, and the consistency index M / S by the rounding of p_distance_text, nan for S = 0"""
    S, M = sum(int(x) for x in steps), sum(int(x) for x in minsteps)
    H = sum(int(a) > int(b) for a, b in zip(steps, minsteps))
    return "# sites=%d steps=%d minsteps=%d homoplasic=%d ci=%s" % (len(steps), S, M, H, p_distance_text(S - M, M))


def core_branches_text(rows, steps, minsteps, gap_open: int = 0, coremin: int = 0) -> bytes:
    """The file of --corebranches: tab-separated; the comment lines of core_partitions_text, the line of
    parsimony_summary, a line of column names, then one line per branch in the order given, numbered from 1.  rows: (the names of the
    files below the branch, its length, its support label or None, its 4 x 4 counts of changes [from][to])."""
    out = _core_comments(gap_open, coremin) + [parsimony_summary(steps, minsteps), "\t".join(CORE_BRANCHES_COLUMNS)]
    for i, (files, length, label, counts) in enumerate(rows):
        changes = sum(int(x) for row in counts for x in row)
        transitions = sum(int(counts[a][b]) for a, b in PARSIMONY_TRANSITIONS)
        out.append("%d\t%s\t%.9f\t%s\t%d\t%d\t%d" % (i + 1, ",".join(files), length, "." if label is None else label, changes, transitions, changes - transitions))
    return ("\n".join(out) + "\n").encode("latin1")


def core_branch_sites_text(site_rows, changes, steps, minsteps, gap_open: int = 0, coremin: int = 0) -> bytes:
    """The file of --corebranchsites: tab-separated; the same comment lines and summary, a line of column names, then
    one line per change in the order given (column, then branch).  site_rows: the rows of core_sites_text, whose fields open the line;
    changes: (site counted from 0, branch counted from 1, code from, code to)."""
    out = _core_comments(gap_open, coremin) + [parsimony_summary(steps, minsteps), "\t".join(CORE_BRANCH_SITES_COLUMNS)]
    for site, branch, a, b in changes:
        block, record, start, end, rev, before = site_rows[site]
        out.append("%d\t%d\t%s\t%d\t%s\t%d\t%s\t%s\t%d\t%d" % (site + 1, block, record, end - before if rev else start + before + 1, "-" if rev else "+", branch,
                                                                 PARSIMONY_BASES[a], PARSIMONY_BASES[b], steps[site], minsteps[site]))
    return ("\n".join(out) + "\n").encode("latin1")


CORE_DENSE_COLUMNS = ("file", "block", "record", "first", "last", "strand", "differences", "first_column", "last_column")


def core_dense_text(rows, window: int, max_diff: int, gap_open: int = 0, coremin: int = 0) -> bytes:
    """The file of --coredense: tab-separated; a line `# densitywindow=W densitymax=T`, a line `# gapopen=N` for
    gap_open > 0, a line `# coremin=M` for coremin > 0, a line of column names, then one line per masked interval in the order BlockFinder.group_mask returns them.  rows:
    (file name of the masked row, block id, record name, start, end, rev, before_first, before_last, differences, first column, last
    column) -- the centre instance of the block (0-based, half-open, on the first file), the centre indices of the interval's first and
    last column, and those columns in the concatenation counted from 0.  Positions are 1-based on the record by the rule of
    core_sites_text -- start + before + 1 forward, end - before on a reverse instance, where the two swap so that first <= last; the
    columns are written 1-based and inclusive."""
    out = ["# densitywindow=%d densitymax=%d" % (window, max_diff)] + _core_comments(gap_open, coremin) + ["\t".join(CORE_DENSE_COLUMNS)]
    for name, block, record, start, end, rev, before_first, before_last, ndiff, first_column, last_column in rows:
        lo, hi = (end - before_last, end - before_first) if rev else (start + before_first + 1, start + before_last + 1)
        out.append("%s\t%d\t%s\t%d\t%d\t%s\t%d\t%d\t%d" % (name, block, record, lo, hi, "-" if rev else "+", ndiff, first_column + 1, last_column + 1))
    return ("\n".join(out) + "\n").encode("latin1")


def core_presence_text(names: Sequence[str], rows: Sequence[Tuple[int, Sequence[bool]]], gap_open: int = 0, coremin: int = 0) -> bytes:
    """The file of --corepresence: tab-separated; the comment lines of core_partitions_text, a line `block` and the
    files' base names, then one line per used block in ascending id: the id and, per input file, 1 where the block has its instance in
    the file and 0 where it has none.  rows: (block id, one flag per file)."""
    out = _core_comments(gap_open, coremin) + ["\t".join(["block"] + list(names))]
    out += ["\t".join(["%d" % block] + ["1" if x else "0" for x in held]) for block, held in rows]
    return ("\n".join(out) + "\n").encode("latin1")


# ------------------------------------------------------------------------------------------ calls from uncovered regions (--uncovered, --unmapped)

CALL_DELETION, CALL_INSERTION, CALL_UNMAPPED = 0, 1, 2      # SBL_CALL_* (include/sibelia_amd.h)
PIECE_LITERAL, PIECE_RECORD = 0, 1                          # SBL_PIECE_*
PIECE_DTYPE = np.dtype([("kind", "<u4"), ("chr", "<u4"), ("start", "<u8"), ("end", "<u8"), ("width", "<u4"), ("pad_", "<u4")])      # sbl_text_piece
LINE_LENGTH = 60                                  # src/csibelia/C-Sibelia.py:19


class TextPieces:
    """The ordered piece list of BlockFinder.spell_text: literal text (kept in one blob; neighbouring literals become one piece) and
    ranges of the original records, which the device spells -- the host never holds an allele."""

    def __init__(self):
        self.literals = bytearray()
        self._pieces = []

    def lit(self, text: bytes) -> None:
        if not text:
            return
        at = len(self.literals)
        self.literals += text
        if self._pieces and self._pieces[-1][0] == PIECE_LITERAL and self._pieces[-1][3] == at:
            self._pieces[-1] = (PIECE_LITERAL, 0, self._pieces[-1][2], at + len(text), 0, 0)
        else:
            self._pieces.append((PIECE_LITERAL, 0, at, at + len(text), 0, 0))

    def rec(self, chr_: int, start: int, end: int, width: int = 0) -> None:
        self._pieces.append((PIECE_RECORD, int(chr_), int(start), int(end), int(width), 0))

    def pieces(self) -> np.ndarray:
        return np.array(self._pieces, dtype=PIECE_DTYPE) if self._pieces else np.zeros(0, dtype=PIECE_DTYPE)


def vcf_pieces(names: Sequence[str], first_size: int, first_base: bytes, records, calls, breakends: bool, gap_open: int = 0) -> TextPieces:
    """The VCF of --variants --uncovered as pieces (C-Sibelia.py:433-463, :575-585): the header; with `breakends` two records
    bnd_<2i> / bnd_<2i + 1> per unmapped insertion i (write_insertions_vcf: on the first reference record at POS 1, REF = `first_base`,
    that record's first base as its file spells it, CIPOS = 0,<first_size>); then all variant records sorted stably by (description,
    POS) -- `records` (those of vcf_text: description, POS, REF, ALT) first in the unsorted list, then the deletions and anchored
    insertions of `calls` (CALL_DTYPE, in record order and ascending start), whose alleles are ranges of the records:
      deletion [s, e) of record c     POS s, REF c[s - 1, e), ALT c[s - 1, s)   (s = 0: REF c[0, e), ALT '.')
      insertion [s, e) at p of r      POS p, REF r[p - 1, p), ALT r[p - 1, p) c[s, e)"""
    t = TextPieces()
    t.lit(("\n".join(vcf_header_lines(names[0], gap_open)) + "\n").encode("latin1"))
    if breakends:
        chrom, ref = strip_chr_id(names[0]), first_base.decode("latin1")
        info = "IMPRECISE;SVTYPE=BND;CIPOS=0,%d" % first_size
        unmapped = [u for u in calls if u["kind"] == CALL_UNMAPPED]
        for i, u in enumerate(unmapped):
            contig = names[int(u["chr"])]
            for j, alt in enumerate(("%s[%s:%d[" % (ref, contig, int(u["start"]) + 1), "]%s:%d]%s" % (contig, int(u["end"]) + 1, ref))):
                t.lit(("\t".join([chrom, "1", "bnd_%d" % (2 * i + j), ref, alt, ".", ".", info]) + "\n").encode("latin1"))
    rows = [(name, pos, ref or b".", alt or b".") for name, pos, ref, alt in records]
    for u in calls:
        c, s, e, r, p = int(u["chr"]), int(u["start"]), int(u["end"]), int(u["ref_chr"]), int(u["pos"])
        if u["kind"] == CALL_DELETION:
            rows.append((names[c], s, (c, s - 1 if s else 0, e), (c, s - 1, s) if s else b"."))
        elif u["kind"] == CALL_INSERTION:
            rows.append((names[r], p, (r, p - 1, p), (r, p - 1, p, c, s, e)))
    for name, pos, ref, alt in sorted(rows, key=lambda x: (x[0], x[1])):
        t.lit(("%s\t%d\t.\t" % (strip_chr_id(name), pos)).encode("latin1"))
        for allele, after in ((ref, b"\t"), (alt, b"\t.\t.\t.\n")):
            if isinstance(allele, bytes):
                t.lit(allele)
            else:
                for k in range(0, len(allele), 3):
                    t.rec(*allele[k:k + 3])
            t.lit(after)
    return t


def unmapped_fasta_pieces(names: Sequence[str], calls) -> TextPieces:
    """write_insertions_fasta (C-Sibelia.py:493-500) as pieces: per unmapped insertion [s, e) of record c the description
    Seq="<description of c>",Start=<s + 1>",End=<e> -- the quote after Start's value is the reference's -- and the bases in lines of 60."""
    t = TextPieces()
    for u in calls:
        if u["kind"] == CALL_UNMAPPED:
            c, s, e = int(u["chr"]), int(u["start"]), int(u["end"])
            t.lit(('>Seq="%s",Start=%d",End=%d\n' % (names[c], s + 1, e)).encode("latin1"))
            t.rec(c, s, e, LINE_LENGTH)
    return t
