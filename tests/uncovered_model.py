"""Model of --uncovered the way the reference's comparison tool does it (src/csibelia/C-Sibelia.py:325-338, :373-427,
:446-463, :493-500): one array cell per base, painted block by block in ascending id, the runs read off the arrays, the texts joined
from Python strings.  It shares nothing with the interval bookkeeping of csrc/uncovered.hip or with the piece lists of
sibelia_amd/formats.py, which are checked against it.

A block list is [(signed id, record, start, end)], 0-based half-open, the sign the strand; `lists` holds the lists of the stages in
order, the last one the final list.  A call is (kind, record, start, end, reference record, position) with kind 'D' (deletion), 'I'
(anchored insertion) or 'U' (unmapped insertion); reference record and position are 0 for 'U'."""
import numpy as np

UNCOVER = 0


def _groups(blocks):
    g = {}
    for b, c, s, e in blocks:
        g.setdefault(abs(b), []).append((b, c, s, e))
    return g


def depict_coverage(blocks, sizes, nref, cover=None):
    if cover is None:
        cover = [np.full(n, UNCOVER, dtype=np.int64) for n in sizes]
    groups = _groups(blocks)
    for block_id in sorted(groups):                 # a Python 2 dict of the dense ids 1..N iterates in ascending order
        instances = groups[block_id]
        reference = [i for i in instances if i[1] < nref]
        if reference and len(reference) < len(instances):
            for _, c, s, e in instances:
                cover[c][s:e] = block_id
    return cover


def determine_unique_block(instances, nref, m):
    if len(instances) == 2:
        ref = next((i for i in instances if i[1] < nref), None)
        asm = next((i for i in instances if i[1] >= nref), None)
        if ref is not None and asm is not None and ref[3] - ref[2] >= m and asm[3] - asm[2] >= m:
            return ref, asm
    return None, None


def uncovered_runs(cover):
    """the maximal runs of UNCOVER cells, read off the array"""
    edge = np.diff(np.concatenate(([0], (cover == UNCOVER).astype(np.int8), [0])))
    return zip(np.flatnonzero(edge == 1).tolist(), np.flatnonzero(edge == -1).tolist())


def calls(lists, sizes, nref, m):
    all_cover = None
    for stage in lists:
        all_cover = depict_coverage(stage, sizes, nref, all_cover)
    main_cover = depict_coverage(lists[-1], sizes, nref)
    final = _groups(lists[-1])
    out = []
    for c, cover in enumerate(all_cover):           # record order (the reference walks a dict of strings: no order of its own)
        for start, end in uncovered_runs(cover):
            if end - start <= m:
                continue
            if c < nref:
                out.append(("D", c, start, end, c, start))
                continue
            call = ("U", c, start, end, 0, 0)
            if start > 0 and main_cover[c][start - 1] != UNCOVER:
                ref, asm = determine_unique_block(final[int(main_cover[c][start - 1])], nref, m)
                if ref is not None:
                    pos = ref[3] if (ref[0] < 0) == (asm[0] < 0) else ref[2]
                    if pos > 0:
                        call = ("I", c, start, end, ref[1], pos)
            out.append(call)
    return out


def strip_chr_id(chr_id):
    part = chr_id.split("|")
    return part[-2].split(".")[0] if len(part) == 5 else chr_id


def bnd_lines(names, seqs, found):
    """write_insertions_vcf for the 'U' calls of `found`: seqs[0][0] is quoted as it stands, lower case included."""
    out = []
    ref = seqs[0][:1].decode()
    info = "IMPRECISE;SVTYPE=BND;CIPOS=0,%d" % len(seqs[0])
    for i, (_, c, s, e, _, _) in enumerate(u for u in found if u[0] == "U"):
        out.append("\t".join([strip_chr_id(names[0]), "1", "bnd_%d" % (2 * i), ref, "%s[%s:%d[" % (ref, names[c], s + 1), ".", ".", info]))
        out.append("\t".join([strip_chr_id(names[0]), "1", "bnd_%d" % (2 * i + 1), ref, "]%s:%d]%s" % (names[c], e + 1, ref), ".", ".", info]))
    return out


def variant_rows(names, seqs, found):
    """[(description, POS, REF, ALT)] of the 'D' and 'I' calls, alleles upper-cased as Variant.__init__ does."""
    out = []
    for kind, c, s, e, r, p in found:
        if kind == "D":
            common = seqs[c][s - 1:s] if s > 0 else b""
            out.append((names[c], s, (common + seqs[c][s:e]).upper().decode(), common.upper().decode() or "."))
        elif kind == "I":
            common = seqs[r][p - 1:p]
            out.append((names[r], p, common.upper().decode(), (common + seqs[c][s:e]).upper().decode()))
    return out


def record_lines(rows):
    """write_variants_vcf after the stable sort by (description, POS)"""
    return ["\t".join([strip_chr_id(n), str(p), ".", ref, alt, ".", ".", "."]) for n, p, ref, alt in sorted(rows, key=lambda x: (x[0], x[1]))]


def unmapped_fasta(names, seqs, found):
    """write_insertions_fasta"""
    out = []
    for kind, c, s, e, _, _ in found:
        if kind == "U":
            out.append('>Seq="%s",Start=%d",End=%d' % (names[c], s + 1, e))
            text = seqs[c][s:e].upper().decode()
            out += [text[o:o + 60] for o in range(0, len(text), 60)]
    return "".join(x + "\n" for x in out).encode()


# ---- the case table of tests/test_uncovered_model.py and tests/test_gpu_uncovered.py: two records of 100 bases, the first one the
# reference set, m = 5.  name -> (lists, the calls worked out by hand)
SIZES, NREF, M = [100, 100], 1, 5
CASES = {
    # a run at a record's start (POS 0, no base before it) and one at its end
    "record_start_and_end": ([[(1, 0, 10, 90), (1, 1, 0, 100)]],
                             [("D", 0, 0, 10, 0, 0), ("D", 0, 90, 100, 0, 90)]),
    # [20, 25) is m long: nothing; [50, 56) is m + 1
    "run_of_m_and_of_m_plus_1": ([[(1, 0, 0, 20), (1, 1, 0, 20), (2, 0, 25, 50), (2, 1, 20, 45), (3, 0, 56, 100), (3, 1, 45, 100)]],
                                 [("D", 0, 50, 56, 0, 50)]),
    # [40, 60) of both records is covered by the first stage only
    "covered_in_an_earlier_stage": ([[(1, 0, 0, 100), (1, 1, 0, 100)], [(1, 0, 0, 40), (1, 1, 0, 40), (2, 0, 60, 100), (2, 1, 60, 100)]],
                                    []),
    # base 49 of record 1 is covered by the first stage only: the run starts behind it, but the FINAL list has no block there
    "anchor_base_covered_only_earlier": ([[(1, 0, 0, 50), (1, 1, 0, 50)], [(1, 0, 0, 40), (1, 1, 0, 40)]],
                                         [("D", 0, 50, 100, 0, 50), ("U", 1, 50, 100, 0, 0)]),
    # both instances off the reference: the block covers nothing
    "block_within_the_assembly": ([[(1, 1, 0, 30), (1, 1, 50, 80)]],
                                  [("D", 0, 0, 100, 0, 0), ("U", 1, 0, 100, 0, 0)]),
    "anchor_same_strand": ([[(1, 0, 10, 50), (1, 1, 0, 40), (2, 0, 50, 100), (2, 1, 80, 100)]],
                           [("D", 0, 0, 10, 0, 0), ("I", 1, 40, 80, 0, 50)]),
    "anchor_both_reverse": ([[(-1, 0, 10, 50), (-1, 1, 0, 40), (2, 0, 50, 100), (2, 1, 80, 100)]],
                            [("D", 0, 0, 10, 0, 0), ("I", 1, 40, 80, 0, 50)]),
    "anchor_opposite_strand": ([[(1, 0, 10, 50), (-1, 1, 0, 40), (2, 0, 50, 100), (2, 1, 80, 100)]],
                               [("D", 0, 0, 10, 0, 0), ("I", 1, 40, 80, 0, 10)]),
    # the reference instance starts at base 0: position 0, no base before it
    "anchor_opposite_strand_at_base_0": ([[(1, 0, 0, 50), (-1, 1, 0, 40), (2, 0, 50, 100), (2, 1, 80, 100)]],
                                         [("U", 1, 40, 80, 0, 0)]),
    "anchor_with_three_instances": ([[(1, 0, 10, 50), (1, 1, 0, 40), (1, 1, 90, 100), (2, 0, 50, 100), (2, 1, 80, 90)]],
                                    [("D", 0, 0, 10, 0, 0), ("U", 1, 40, 80, 0, 0)]),
    "anchor_instance_shorter_than_m": ([[(1, 0, 10, 13), (1, 1, 0, 40), (2, 0, 13, 100), (2, 1, 80, 100)]],
                                       [("D", 0, 0, 10, 0, 0), ("U", 1, 40, 80, 0, 0)]),
    "anchor_instance_of_exactly_m": ([[(1, 0, 10, 15), (1, 1, 0, 40), (2, 0, 15, 100), (2, 1, 80, 100)]],
                                     [("D", 0, 0, 10, 0, 0), ("I", 1, 40, 80, 0, 15)]),
    # blocks 3 and 1 both hold base 39 of record 1; block 1 starts later there, block 3 is the last writer
    "largest_id_wins": ([[(3, 0, 60, 90), (3, 1, 0, 40), (1, 0, 10, 50), (1, 1, 30, 40), (2, 0, 90, 100), (2, 1, 80, 100)]],
                        [("D", 0, 0, 10, 0, 0), ("D", 0, 50, 60, 0, 50), ("I", 1, 40, 80, 0, 90)]),
    "empty_list": ([[]],
                   [("D", 0, 0, 100, 0, 0), ("U", 1, 0, 100, 0, 0)]),
    # ... and the anchor's position is the reference record's size: the base before it is its last one
    "empty_stage_before_the_final_list": ([[], [(1, 0, 0, 100), (1, 1, 0, 94)]],
                                          [("I", 1, 94, 100, 0, 100)]),
}


def parse_blocks_coords(text):
    """blocks_coords.txt -> [(signed id, record, start, end)], 0-based half-open"""
    out, block = [], None
    for line in text.splitlines():
        if line.startswith("Block #"):
            block = int(line[7:])
            continue
        f = line.split("\t")
        if block is None or len(f) != 5 or f[1] not in "+-" or not f[0].isdigit():
            continue
        c, a, b = int(f[0]) - 1, int(f[2]), int(f[3])
        out.append((block, c, a - 1, b) if f[1] == "+" else (-block, c, b - 1, a))
    return out
