"""The whole pipeline of the reference's program (reference src/sibelia.cpp:186-345) over BlockFinder.

`parse_args` reads the reference's command line, `run` restates its main: the stage cascade with the trimK / lastK rule, the
per-stage blocks of --allstages / -v (computed BEFORE the stage: they consume the rand() stream), the rand() stream kept in step
with and without -r, and the choice of which files are written.  `run` returns (return code, {relative file name: bytes}, text for
standard output); `main` writes the files and prints the text (python -m sibelia_amd).

--maf / --variants (two input files) add what the reference's comparison tool C-Sibelia.py makes of such a run: the alignments of the
unique blocks in MAF and the variants read off them in VCF (`align_unique_blocks`).  --gapopen N gives those alignments and the ones of
--multimaf an affine gap cost (N for opening a gap run); --wideband aligns the blocks whose band is beyond the LDS band
classes instead of leaving them out.  --multimaf (any number of input files) writes a
multiple alignment of every block with at least two instances (`align_block_groups`); --multivariants (two or more input files) reads
the calls off those alignments for the blocks with one instance in the first file and at most one in each other file and writes them as
a multi-sample VCF.  --distances / --distancecounts (two or more input files) count, on the same alignments, the matches,
mismatches and gaps between every two input files over the blocks with at most one instance in each file, on the device, and write a
distance matrix and the counts behind it.  --corealignment / --corepartitions / --coresnps / --coresites (two or more
input files) concatenate, on the device, the same alignments of the blocks with exactly one instance in every file into the core-genome
alignment and its variable columns, one FASTA record per input file, with the tables that say where a block and a column come from
(DESIGN.md 0.9).  --corefiltered / --corefilteredsnps / --corefilteredsites / --coredense (two or more input files) make the same files from
the rows with every file's SNP-dense regions -- more than --densitymax differences from the first file within --densitywindow of its
bases -- replaced by N, and the table of those regions; the mask is computed on the device.  --coremin M
turns the core of all of these into the soft core -- blocks with instances in at least M files, gaps for the files without one -- and
--corepresence lists which files every used block is in.  --coretree /
--corefilteredtree (three or more input files) write the neighbour-joining tree of the input files from the variable columns of those
two alignments in Newick format, with --bootstrap B the support of B replicates whose pair counts are made on the device (DESIGN.md 0.11;
`tree.py`).  --coreconsensus / --corefilteredconsensus write the majority-rule consensus of those B replicate trees and --coreboottrees /
--corefilteredboottrees the replicate trees themselves; all B + 1 matrices of a run are joined on the device in one call, up to 64 input
files.  --corebranches / --corebranchsites / --coresnptree and their
--corefiltered... twins (three to 64 input files) map the columns of --coresnps onto the branches of that tree by Fitch parsimony on the
device: a table of the branches with their changes, a table of the changes, and the tree with the changes as lengths.
--uncovered adds the rest of C-Sibelia's VCF to
the file of --variants: the deletions and insertions read off the regions no block covers and the breakend records of the insertions
that cannot be placed (--unmapped FILE: those as FASTA instead); the alleles are spelled on the device (`uncovered_files`).

Not written: circos/ and d3_blocks_diagram.html -- the reference instantiates them from templates embedded in its own sources.

Everything up to `run` (option parsing, stage files, the k rule, the file plan) imports and works without the HIP library.
"""
from __future__ import annotations

import argparse
import os
import re
import sys
from typing import Callable, Dict, List, Optional, Sequence, Tuple

INT_MAX = 2 ** 31 - 1
MAX_INPUT_SIZE = 1 << 30                      # src/common.h:52

# the parameter sets of src/util.cpp:52-87: (vertex size k, minimum branch size) per stage
PARAMETER_SETS = {
    "loose": [(30, 150), (100, 1000), (1000, 5000), (5000, 15000)],
    "fine": [(30, 150), (100, 500), (500, 1500)],
    "far": [(15, 120), (100, 500), (500, 1500)],
}

ALIGN_HELP = ("Blocks that are not unique -- more or fewer than two instances, or not one in each input file -- are not aligned here: "
              "the reference's comparison tool hands them to mlagan.  See --multimaf.")

MULTI_HELP = ("Any number of input files: align every synteny block with at least two instances, all of its instances, base by base on the "
              "device and write one MAF paragraph per block.  The alignment is centre-star on the block's first instance (by record, start, "
              "end, strand): every other instance is aligned to it as under --maf and the gaps are merged.  It is this program's own "
              "definition, not mlagan's, which the reference's comparison tool runs on such blocks.")

MULTIVARIANTS_HELP = ("Two or more input files: write the SNVs and indels read off the multiple alignments of --multimaf in VCF format, one sample "
                      "column per input file after the first (named by the file's base name; positions on the records of the first file).  A "
                      "block is used if all its instances are at least the minimum block size long, exactly one of them lies in the first file "
                      "and at most one in each other file; a file without an instance gets the genotype '.'.")

DISTANCES_HELP = ("Two or more input files: write the p-distance of every two input files -- mismatches / (matches + mismatches) over the aligned "
                  "columns in which both hold one of A C G T -- as a square matrix in PHYLIP format, the files named by their base names.  The "
                  "columns are those of the multiple alignments of --multimaf; a block is used if it has at least two instances, all at least "
                  "the minimum block size long, and at most one in each file.  No correction for multiple substitutions; 'nan' where two "
                  "files share no such column.")

DISTANCECOUNTS_HELP = ("Two or more input files: write the counts behind --distances as tab-separated text, one line per pair of input files: the "
                       "blocks used, matches, mismatches, ambiguous columns (a base code other than A C G T on either side) and the bases of "
                       "each file opposite a gap of the other.")

COREALIGNMENT_HELP = ("Two or more input files: write the core-genome alignment in FASTA format -- the multiple alignments of --multimaf of the "
                      "core blocks, one after the other in ascending block id, one record per input file (named by the file's base name), 80 "
                      "columns per line.  A block is a core block if it has exactly one instance in every input file, all at least the "
                      "minimum block size long.  The text is put together on the device.")

COREPARTITIONS_HELP = ("Two or more input files: write the columns every core block takes in the alignment of --corealignment as tab-separated "
                       "text: block, first and last column, counted from 1.")

CORESNPS_HELP = ("Two or more input files: write the variable columns of the core-genome alignment in FASTA format, as --corealignment does: "
                 "the columns in which every file holds one of A C G T and not all hold the same.")

CORESITES_HELP = ("Two or more input files: write where every column of --coresnps comes from as tab-separated text: column, block, record "
                  "of the first file, 1-based position on it and strand of the block's instance there.")

COREFILTERED_HELP = ("Two or more input files: write the core-genome alignment of --corealignment with, in every file's record, the regions "
                     "in which it differs from the first file more densely than --densitymax in --densitywindow replaced by N (gaps stay).  "
                     "The columns are those of --corealignment, so --corepartitions describes this file too.  Such regions are "
                     "typical of imported DNA (recombination, phage) and of misassembled repeats; SNP pipelines drop them before a tree "
                     "is built.  The mask is computed on the device.")

COREFILTEREDSNPS_HELP = ("Two or more input files: write the variable columns of the alignment of --corefiltered, as --coresnps does.  N is not "
                         "one of A C G T, so a column masked in any file is dropped for all files.")

COREFILTEREDSITES_HELP = "Two or more input files: write where every column of --corefilteredsnps comes from, as --coresites does."

COREDENSE_HELP = ("Two or more input files: write the masked regions as tab-separated text, one line per region: the masked file, block, "
                  "record of the first file with the first and last 1-based position of the region on it and the strand of the block's "
                  "instance there, the differences inside, and the first and last column in the alignment of --corealignment, counted from 1.")

DENSITY_MAX = 2 ** 32 - 1
DENSITYWINDOW_DEFAULT, DENSITYMAX_DEFAULT = 1000, 3      # the defaults of CFSAN's SNP pipeline: a convention, not a measurement
DENSITYWINDOW_HELP = ("With --corefiltered, --corefilteredsnps, --corefilteredsites or --coredense: the window of the density filter in bases of "
                      "the first file, 1 .. 4294967295, default 1000.")
DENSITYMAX_HELP = ("With the same options: the differences a window may hold, 1 .. 4294967295, default 3: a region is masked where more than "
                   "this many differences lie within one window.")

CORETREE_HELP = ("Three or more input files: write the neighbour-joining tree of the input files in Newick format, one line, the files named "
                 "by their base names.  The distance of two files is the number of columns of --coresnps in which they differ over the number "
                 "of columns of --corealignment in which every file holds one of A C G T (--treemodel).  The tree is unrooted and written "
                 "from the node next to the first file, branch lengths with 9 decimals.  Not written where there is no such column.")
COREFILTEREDTREE_HELP = "Three or more input files: write the same tree from the alignment of --corefiltered, its dense regions masked."
BOOTSTRAP_MAX = 100000
BOOTSTRAP_HELP = ("With --coretree or --corefilteredtree, or with the consensus and replicate tree files, which are made of the replicates: label every inner branch with the percentage of B bootstrap replicates that hold it, "
                  "0 .. 100000, default 0: no labels.  A replicate draws as many columns as --coresnps has, with replacement; the counts of "
                  "all replicates are made on the device.")
BOOTSEED_MAX = 2 ** 64 - 1
BOOTSEED_HELP = "With the same options: the seed of the draws, 0 .. 18446744073709551615, default 1.  The same seed gives the same file."
TREEMODEL_HELP = ("With the same options: p, the proportion of differing columns (default), or jc, Jukes and Cantor's correction "
                  "-3/4 ln(1 - 4p/3); a tree with two files at p >= 0.75 is then not written.")

CORECONSENSUS_HELP = ("Three or more input files, with --bootstrap B of 1 or more: write the majority-rule consensus of the B replicate trees of "
                      "--coretree in Newick format, one line: the branches that more than half of the replicates hold, each labelled with the "
                      "percentage that holds it and as long as its mean length in those replicates.  Without such a branch the tree is a star.  "
                      "The replicate trees are built on the device for up to 64 input files.")
COREFILTEREDCONSENSUS_HELP = "The same consensus from the replicates of --corefilteredtree."
COREBOOTTREES_HELP = ("Three or more input files, with --bootstrap B of 1 or more: write the B replicate trees of --coretree in Newick format, one "
                      "line each in the order of the replicates, without labels: the input of an external consensus or summary program.")
COREFILTEREDBOOTTREES_HELP = "The same replicate trees from the replicates of --corefilteredtree."

PARSIMONY_MAX_FILES = 64
COREBRANCHES_HELP = ("Three to 64 input files: map the columns of --coresnps onto the tree of --coretree by Fitch parsimony, on the device, and write "
                     "one line per branch as tab-separated text, in the order the tree's text visits them: its number, the files below it, its "
                     "length and support as in --coretree ('.' on a branch to a file and without --bootstrap), and the changes it carries, split "
                     "into transitions (A-G, C-T) and transversions.  The tree is read from the first file; where several bases are equally "
                     "good for an inner node it takes its parent's, else the first of A C T G.  A comment line gives the sites, their steps, the "
                     "least their bases allow, the homoplasic sites (more steps than that) and the consistency index.  Not written "
                     "where --coretree is not.")
COREFILTEREDBRANCHES_HELP = "The same table from the columns of --corefilteredsnps on the tree of --corefilteredtree."
COREBRANCHSITES_HELP = ("Three to 64 input files: write the changes themselves as tab-separated text, one line per change by column, then branch: "
                        "the column's fields of --coresites, the branch as numbered in --corebranches, the base on the side of the first file, "
                        "the base on the other side, and the column's steps and least steps.")
COREFILTEREDBRANCHSITES_HELP = "The same table for --corefilteredsnps, its leading fields those of --corefilteredsites."
CORESNPTREE_HELP = ("Three to 64 input files: write the tree of --coretree, same order and support labels, with every branch as long as the "
                    "number of changes it carries: a SNP-scaled tree.")
COREFILTEREDSNPTREE_HELP = "The same tree from --corefilteredtree and --corefilteredsnps."

COREMIN_HELP = ("With any of the --core..., --corefiltered... and tree options or --corepresence: the soft core.  Use the blocks with instances "
                "in at least M input files, 2 .. the number of files, default the number of files: the strict core.  Below it a block is "
                "used if all its instances are at least the minimum block size long, exactly one lies in the first file, at most one in "
                "each other file and they reach at least M files.  A file without an instance of a block gets gaps in the alignments; "
                "a column counts as variable or as comparable by the files that are there, and a tree takes the distance of two files "
                "over the columns of the blocks that both have.  A tree is not written where two files share no such column.  "
                "The tab-separated files record M in a line `# coremin=M`.")
COREPRESENCE_HELP = ("Two or more input files: write which input files every used block has an instance in as tab-separated text: a line "
                     "`block` and the files' base names, then the block and 1 or 0 per file, in ascending block id.")

CORE_OPTIONS = (("--corealignment", "corealignment"), ("--corepartitions", "corepartitions"), ("--coresnps", "coresnps"), ("--coresites", "coresites"))
DENSITY_OPTIONS = (("--corefiltered", "corefiltered"), ("--corefilteredsnps", "corefilteredsnps"), ("--corefilteredsites", "corefilteredsites"), ("--coredense", "coredense"))
TREE_OPTIONS = (("--coretree", "coretree"), ("--corefilteredtree", "corefilteredtree"))
PRESENCE_OPTIONS = (("--corepresence", "corepresence"),)
# the options that name a file made from alignments, as (flag, attribute) in the order the files are written; those that read the
# multiple alignments of the blocks (align_block_groups); those of them that compare the input files by their names
FILE_OPTIONS = (("--maf", "maf"), ("--variants", "variants"), ("--unmapped", "unmapped"), ("--multimaf", "multimaf"), ("--multivariants", "multivariants"),
                ("--distances", "distances"), ("--distancecounts", "distancecounts")) + CORE_OPTIONS + DENSITY_OPTIONS + PRESENCE_OPTIONS + TREE_OPTIONS
# the files made of the bootstrap replicates' trees, written after all of those: the consensus of the plain and of the masked rows, then the
# replicate trees of the two.  ROWS_TREE_OPTIONS: per kind of rows its tree, consensus and replicate trees
REPLICATE_OPTIONS = (("--coreconsensus", "coreconsensus"), ("--corefilteredconsensus", "corefilteredconsensus"),
                     ("--coreboottrees", "coreboottrees"), ("--corefilteredboottrees", "corefilteredboottrees"))
# the files of the parsimony mapping on the tree, written after all of those: the branch tables of the plain and of the
# masked rows, then the change tables, then the SNP-scaled trees.  ROWS_BRANCH_OPTIONS: per kind of rows its three
BRANCH_OPTIONS = (("--corebranches", "corebranches"), ("--corefilteredbranches", "corefilteredbranches"),
                  ("--corebranchsites", "corebranchsites"), ("--corefilteredbranchsites", "corefilteredbranchsites"),
                  ("--coresnptree", "coresnptree"), ("--corefilteredsnptree", "corefilteredsnptree"))
ALL_TREE_OPTIONS = TREE_OPTIONS + REPLICATE_OPTIONS + BRANCH_OPTIONS
ROWS_TREE_OPTIONS = {False: (TREE_OPTIONS[0], REPLICATE_OPTIONS[0], REPLICATE_OPTIONS[2]), True: (TREE_OPTIONS[1], REPLICATE_OPTIONS[1], REPLICATE_OPTIONS[3])}
ROWS_BRANCH_OPTIONS = {False: BRANCH_OPTIONS[0::2], True: BRANCH_OPTIONS[1::2]}
ALL_FILE_OPTIONS = FILE_OPTIONS + REPLICATE_OPTIONS
GROUP_OPTIONS, NAMED_FILE_OPTIONS = ALL_FILE_OPTIONS[3:], ALL_FILE_OPTIONS[5:]
# ... and with the files of the mapping: every file made from alignments, in the order they are written
EVERY_FILE_OPTIONS = ALL_FILE_OPTIONS + BRANCH_OPTIONS

UNCOVERED_HELP = ("With --variants and --allstages: add what the reference's comparison tool calls from the regions that no block with an "
                  "instance in both input files covers, at any stage: a region of the first file longer than the minimum block size as "
                  "a deletion, such a region of the second file as an insertion behind the unique block that ends before it, and "
                  "where there is no such block as two breakend records (bnd_<n>).")

GAPOPEN_MAX = 100000
GAPOPEN_HELP = ("With --maf, --variants, --multimaf or --multivariants: the cost of opening a gap run in their alignments, 0 .. 100000, default 0.  A run of L gap "
                "columns costs N + 75 L (match +25, mismatch -75), so that one insertion or deletion is reported as one run, not as pieces "
                "around stray matches.  The files record a value above 0 in a header line.  Not applied to --correctboundaries, whose "
                "alignment is the reference program's own.")

WIDEBAND_HELP = ("With --maf, --variants, --multimaf or --multivariants: also align the blocks whose instances differ in length by more than "
                 "the score diagonal in on-chip memory holds (about 12000 bases, 4800 with --gapopen), with the score diagonal in device memory; "
                 "without it such a block is named on standard error and left out.  The alignments themselves are the same, so the "
                 "files record nothing about it.")

NOT_WRITTEN = ("The Circos files (circos/) and d3_blocks_diagram.html of the reference program are not written: "
               "they are instantiated from templates embedded in the reference's sources.")


class PipelineError(RuntimeError):
    """What the reference's main reports as `error: <message>` with return code 1."""


# ------------------------------------------------------------------------------------------ stage files

def parse_stage_text(text: str) -> List[Tuple[int, int]]:
    """ReadStageFile (src/util.cpp:11-50) on the file's text: a count, then `count` pairs of integers, all separated by blanks;
    what follows the last pair is ignored, as a C++ stream extraction leaves it unread."""
    tokens = text.split()
    at = 0

    def take() -> Optional[int]:
        nonlocal at
        if at >= len(tokens):
            return None
        m = re.match(r"[+-]?\d+", tokens[at])       # operator>>(int) reads the longest integer prefix and fails without one
        if not m:
            at = len(tokens)                        # a failed extraction leaves the stream failed: every later read fails too
            return None
        if m.end() == len(tokens[at]):
            at += 1
        else:
            tokens[at] = tokens[at][m.end():]       # the rest of the token stays in the stream
        v = int(m.group())
        if not -2 ** 31 <= v <= INT_MAX:            # out of range for int: the extraction fails
            at = len(tokens)
            return None
        return v

    count = take()
    if count is None:
        raise PipelineError("cannot read stage file")
    if count < 0:
        raise PipelineError("number of stages must be nonnegative")
    stages = []
    for _ in range(count):
        k = take()
        d = take() if k is not None else None
        if k is None or d is None:
            raise PipelineError("too few records in the stage file")
        if k < 2:
            raise PipelineError("vertex size in stage record must be at least 2")
        if d < 0:
            raise PipelineError("minimum branch size in stage record must be nonnegative")
        stages.append((k, d))
    return stages


def read_stage_file(path: str) -> List[Tuple[int, int]]:
    try:
        with open(path, "r", errors="replace") as f:
            text = f.read()
    except OSError:
        raise PipelineError("cannot open stage file")
    return parse_stage_text(text)


# ------------------------------------------------------------------------------------------ command line

class _Parser(argparse.ArgumentParser):
    def error(self, message):                       # TCLAP's ArgException: reported by main, return code 1
        raise PipelineError(message)


def _greater_than(bound: int) -> Callable[[str], int]:
    def conv(s: str) -> int:
        v = int(s)
        if v <= bound:
            raise argparse.ArgumentTypeError("integer > %d expected" % bound)
        return v
    return conv


def _unsigned(s: str) -> int:
    v = int(s)
    if v < 0 or v > 2 ** 32 - 1:
        raise argparse.ArgumentTypeError("unsigned integer expected")
    return v


def _gap_open(s: str) -> int:
    v = int(s)
    if v < 0 or v > GAPOPEN_MAX:
        raise argparse.ArgumentTypeError("integer from 0 to %d expected" % GAPOPEN_MAX)
    return v


def _density(s: str) -> int:
    v = int(s)
    if v < 1 or v > DENSITY_MAX:
        raise argparse.ArgumentTypeError("integer from 1 to %d expected" % DENSITY_MAX)
    return v


def _bounded(lo: int, hi: int):
    def conv(s: str) -> int:
        v = int(s)
        if v < lo or v > hi:
            raise argparse.ArgumentTypeError("integer from %d to %d expected" % (lo, hi))
        return v
    return conv


def build_parser() -> argparse.ArgumentParser:
    p = _Parser(prog="python -m sibelia_amd", description="Program for finding synteny blocks in closely related genomes "
                "(Sibelia 3.0.7's command line over the MI355X library).  " + NOT_WRITTEN)
    p.add_argument("-s", "--parameters", choices=sorted(PARAMETER_SETS), default=None,
                   help="Parameters set, used for the simplification. Option \"loose\" produces fewer blocks, but they are larger (\"fine\" is opposite).")
    p.add_argument("-k", "--stagefile", default=None, metavar="file name", help="File that contains manually chosen simplifications parameters.")
    p.add_argument("-i", "--maxiterations", type=_greater_than(0), default=4, help="Maximum number of iterations during a stage of simplification, default = 4.")
    p.add_argument("-m", "--minblocksize", type=_unsigned, default=5000, help="Minimum size of a synteny block, default value = 5000 BP.")
    p.add_argument("-a", "--sharedonly", action="store_true", help="Output only blocks that occur exactly once in each input sequence.")
    p.add_argument("-r", "--inram", action="store_true", help="Perform all computations in RAM, don't create temp files.")
    p.add_argument("-t", "--tempdir", default=None, metavar="dir name", help="Directory where temporary files are stored.")
    p.add_argument("-o", "--outdir", default=".", metavar="dir name", help="Directory where output files are written")
    p.add_argument("-g", "--graphfile", action="store_true", help="Output resulting condensed de Bruijn graph (in dot format).")
    p.add_argument("-q", "--sequencesfile", action="store_true", help="Output sequences of synteny blocks (FASTA format).")
    p.add_argument("-v", "--visualize", action="store_true", help="Compute the blocks of every stage, as the reference does for its hierarchy diagram (the diagram itself is not written).")
    p.add_argument("--allstages", action="store_true", help="Output coordinates of synteny blocks from all stages")
    p.add_argument("--gff", action="store_true", help="Use GFF format for reporting blocks coordinates")
    p.add_argument("--lastk", type=_greater_than(1), default=None, help="Value of K used for the synteny blocks inferring.")
    p.add_argument("--nopostprocess", action="store_true", help="Do not perform postprocessing (stripe gluing).")
    p.add_argument("--noblocks", action="store_true", help="Do not compute synteny blocks")
    p.add_argument("--correctboundaries", action="store_true", help="Correct boundaries of unique synteny blocks.")
    p.add_argument("--maf", default=None, metavar="FILE", help="Two input files: align the two instances of every unique synteny block base by base "
                   "on the device and write the alignments in MAF format.  " + ALIGN_HELP)
    p.add_argument("--variants", default=None, metavar="FILE", help="Two input files: write the SNVs and indels read off those alignments in VCF format "
                   "(positions on the records of the first file).")
    p.add_argument("--uncovered", action="store_true", help=UNCOVERED_HELP)
    p.add_argument("--unmapped", default=None, metavar="FILE", help="With --uncovered: write the insertions that cannot be placed to FILE in FASTA format "
                   "instead of as breakend records.")
    p.add_argument("--multimaf", default=None, metavar="FILE", help=MULTI_HELP)
    p.add_argument("--multivariants", default=None, metavar="FILE", help=MULTIVARIANTS_HELP)
    p.add_argument("--distances", default=None, metavar="FILE", help=DISTANCES_HELP)
    p.add_argument("--distancecounts", default=None, metavar="FILE", help=DISTANCECOUNTS_HELP)
    p.add_argument("--corealignment", default=None, metavar="FILE", help=COREALIGNMENT_HELP)
    p.add_argument("--corepartitions", default=None, metavar="FILE", help=COREPARTITIONS_HELP)
    p.add_argument("--coresnps", default=None, metavar="FILE", help=CORESNPS_HELP)
    p.add_argument("--coresites", default=None, metavar="FILE", help=CORESITES_HELP)
    p.add_argument("--corefiltered", default=None, metavar="FILE", help=COREFILTERED_HELP)
    p.add_argument("--corefilteredsnps", default=None, metavar="FILE", help=COREFILTEREDSNPS_HELP)
    p.add_argument("--corefilteredsites", default=None, metavar="FILE", help=COREFILTEREDSITES_HELP)
    p.add_argument("--coredense", default=None, metavar="FILE", help=COREDENSE_HELP)
    p.add_argument("--densitywindow", type=_density, default=None, metavar="W", help=DENSITYWINDOW_HELP)
    p.add_argument("--densitymax", type=_density, default=None, metavar="T", help=DENSITYMAX_HELP)
    p.add_argument("--coretree", default=None, metavar="FILE", help=CORETREE_HELP)
    p.add_argument("--corefilteredtree", default=None, metavar="FILE", help=COREFILTEREDTREE_HELP)
    p.add_argument("--coreconsensus", default=None, metavar="FILE", help=CORECONSENSUS_HELP)
    p.add_argument("--corefilteredconsensus", default=None, metavar="FILE", help=COREFILTEREDCONSENSUS_HELP)
    p.add_argument("--coreboottrees", default=None, metavar="FILE", help=COREBOOTTREES_HELP)
    p.add_argument("--corefilteredboottrees", default=None, metavar="FILE", help=COREFILTEREDBOOTTREES_HELP)
    p.add_argument("--corebranches", default=None, metavar="FILE", help=COREBRANCHES_HELP)
    p.add_argument("--corefilteredbranches", default=None, metavar="FILE", help=COREFILTEREDBRANCHES_HELP)
    p.add_argument("--corebranchsites", default=None, metavar="FILE", help=COREBRANCHSITES_HELP)
    p.add_argument("--corefilteredbranchsites", default=None, metavar="FILE", help=COREFILTEREDBRANCHSITES_HELP)
    p.add_argument("--coresnptree", default=None, metavar="FILE", help=CORESNPTREE_HELP)
    p.add_argument("--corefilteredsnptree", default=None, metavar="FILE", help=COREFILTEREDSNPTREE_HELP)
    p.add_argument("--coremin", type=_unsigned, default=None, metavar="M", help=COREMIN_HELP)
    p.add_argument("--corepresence", default=None, metavar="FILE", help=COREPRESENCE_HELP)
    p.add_argument("--bootstrap", type=_bounded(0, BOOTSTRAP_MAX), default=None, metavar="B", help=BOOTSTRAP_HELP)
    p.add_argument("--bootseed", type=_bounded(0, BOOTSEED_MAX), default=None, metavar="S", help=BOOTSEED_HELP)
    p.add_argument("--treemodel", choices=("p", "jc"), default=None, help=TREEMODEL_HELP)
    p.add_argument("--gapopen", type=_gap_open, default=None, metavar="N", help=GAPOPEN_HELP)
    p.add_argument("--wideband", action="store_true", help=WIDEBAND_HELP)
    p.add_argument("--device", type=int, default=-1, metavar="N", help="HIP device to run on (default: the current one)")
    p.add_argument("filenames", nargs="+", metavar="fasta", help="FASTA file(s) with nucleotide sequences.")
    return p


def parse_args(argv: Sequence[str]) -> argparse.Namespace:
    """The reference's options by letter and name; exactly one of -s / -k (TCLAP xorAdd, src/sibelia.cpp:184)."""
    opt = build_parser().parse_args(list(argv))
    if (opt.parameters is None) == (opt.stagefile is None):
        raise PipelineError("exactly one of -s (--parameters) and -k (--stagefile) is required")
    if opt.correctboundaries and len(opt.filenames) != 2:      # src/sibelia.cpp:203-206, before any file is read
        raise PipelineError("In correction mode only two FASTA files are acceptable")
    if opt.maf is not None or opt.variants is not None:
        if len(opt.filenames) != 2:                            # before any file is read
            raise PipelineError("In alignment mode only two FASTA files are acceptable")
        if opt.noblocks:
            raise PipelineError("--maf and --variants need the synteny blocks: they cannot be combined with --noblocks")
    if opt.multimaf is not None and opt.noblocks:
        raise PipelineError("--multimaf needs the synteny blocks: it cannot be combined with --noblocks")
    if opt.multivariants is not None:
        if len(opt.filenames) < 2:                             # before any file is read
            raise PipelineError("--multivariants compares files: it needs at least two")
        if opt.noblocks:
            raise PipelineError("--multivariants needs the synteny blocks: it cannot be combined with --noblocks")
        samples = sample_names(opt.filenames)
        for a in sorted(set(samples)):
            if samples.count(a) > 1:
                raise PipelineError("--multivariants names a sample by its file's base name: two files are called %s" % a)
    for o, _ in _given(opt, NAMED_FILE_OPTIONS + BRANCH_OPTIONS):
        if len(opt.filenames) < 2:                             # before any file is read
            raise PipelineError("%s compares files: it needs at least two" % o)
        if opt.noblocks:
            raise PipelineError("%s needs the synteny blocks: it cannot be combined with --noblocks" % o)
        names = file_names(opt.filenames)
        for a in sorted(set(names)):
            if names.count(a) > 1:
                raise PipelineError("%s names a file by its base name: two files are called %s" % (o, a))
        if o == "--distances":
            for a in names:
                if a != "".join(a.split()):
                    raise PipelineError("--distances writes PHYLIP, which separates by blanks: the file name '%s' holds white space" % a)
    for o, _ in _given(opt, ALL_TREE_OPTIONS):
        if len(opt.filenames) < 3:                             # two files have one distance and no tree
            raise PipelineError("%s builds a tree: it needs at least three input files" % o)
        from . import tree
        try:
            tree.check_names(file_names(opt.filenames))
        except ValueError as e:
            raise PipelineError("%s names a file by its base name: %s" % (o, e))
    for o, _ in _given(opt, BRANCH_OPTIONS):
        if len(opt.filenames) > PARSIMONY_MAX_FILES:           # before anything runs: the mapping on the device takes 64-bit file masks
            raise PipelineError("%s maps the changes onto the tree on the device, which takes at most %d input files: %d are given" % (o, PARSIMONY_MAX_FILES, len(opt.filenames)))
    for o, v in (("--bootstrap", opt.bootstrap), ("--bootseed", opt.bootseed), ("--treemodel", opt.treemodel)):
        if v is not None and not tree_wanted(opt):
            raise PipelineError("%s is a setting of the tree: it needs at least one of --coretree and --corefilteredtree" % o)
    for o, _ in _given(opt, REPLICATE_OPTIONS):
        if not opt.bootstrap:
            raise PipelineError("%s is made of the trees of the bootstrap replicates: it needs --bootstrap B with B of 1 or more" % o)
    opt.bootstrap = opt.bootstrap or 0
    opt.bootseed = 1 if opt.bootseed is None else opt.bootseed
    opt.treemodel = opt.treemodel or "p"
    if opt.uncovered and opt.variants is None:
        raise PipelineError("--uncovered adds its records to the file of --variants: it needs --variants")
    if opt.uncovered and not opt.allstages:
        raise PipelineError("--uncovered reads the blocks of every stage: it needs --allstages")
    if opt.unmapped is not None and not opt.uncovered:
        raise PipelineError("--unmapped takes the insertions that --uncovered finds: it needs --uncovered")
    for o, v in (("--densitywindow", opt.densitywindow), ("--densitymax", opt.densitymax)):
        if v is not None and not density_wanted(opt):
            raise PipelineError("%s sets the density filter: it needs at least one of --corefiltered, --corefilteredsnps, --corefilteredsites and --coredense" % o)
    if opt.coremin is not None:
        if not concat_wanted(opt):
            raise PipelineError("--coremin sets which blocks the core-genome files are made of: it needs at least one of the --core..., "
                                "--corefiltered... and tree options and --corepresence")
        if not 2 <= opt.coremin <= len(opt.filenames):
            raise PipelineError("--coremin is the number of input files a block must reach: 2 .. %d for these input files" % len(opt.filenames))
    else:
        opt.coremin = len(opt.filenames)
    opt.densitywindow = opt.densitywindow or DENSITYWINDOW_DEFAULT
    opt.densitymax = opt.densitymax or DENSITYMAX_DEFAULT
    aligns = bool(_given(opt, EVERY_FILE_OPTIONS))    # --unmapped is given with --variants only
    if opt.gapopen is not None and not aligns:
        raise PipelineError("--gapopen sets a cost of the alignments: it needs at least one of --maf, --variants and --multimaf")
    opt.gapopen = opt.gapopen or 0                  # not given: 0, the linear gap cost
    if opt.wideband and not aligns:
        raise PipelineError("--wideband widens the bands of the alignments: it needs at least one of --maf, --variants, --multimaf and --multivariants")
    if aligns:
        _check_alignment_files(opt)
    return opt


def sample_names(filenames: Sequence[str]) -> List[str]:
    """The sample columns of --multivariants: one per input file after the first, named by the file's base name."""
    return [os.path.basename(os.path.normpath(f)) for f in filenames[1:]]


def file_names(filenames: Sequence[str]) -> List[str]:
    """The names of --distances / --distancecounts: one per input file, the first included, the file's base name."""
    return [os.path.basename(os.path.normpath(f)) for f in filenames]


def _given(opt: argparse.Namespace, options) -> List[Tuple[str, str]]:
    """(flag, file) of those of `options` ((flag, attribute) pairs) that are given, in their order."""
    return [(o, getattr(opt, a)) for o, a in options if getattr(opt, a) is not None]


def core_wanted(opt: argparse.Namespace) -> bool:
    """One of --corealignment / --corepartitions / --coresnps / --coresites is given."""
    return bool(_given(opt, CORE_OPTIONS))


def density_wanted(opt: argparse.Namespace) -> bool:
    """One of --corefiltered / --corefilteredsnps / --corefilteredsites / --coredense is given, or --corefilteredtree, --corefilteredconsensus,
    --corefilteredboottrees or one of --corefilteredbranches / --corefilteredbranchsites / --corefilteredsnptree, which read the same masked rows."""
    return bool(_given(opt, DENSITY_OPTIONS)) or bool(_given(opt, ROWS_TREE_OPTIONS[True] + ROWS_BRANCH_OPTIONS[True]))


def tree_wanted(opt: argparse.Namespace) -> bool:
    """One of --coretree / --corefilteredtree, of the four files made of their replicates or of the six of the parsimony mapping is given."""
    return bool(_given(opt, ALL_TREE_OPTIONS))


def presence_wanted(opt: argparse.Namespace) -> bool:
    """--corepresence is given."""
    return bool(_given(opt, PRESENCE_OPTIONS))


def concat_wanted(opt: argparse.Namespace) -> bool:
    """One of the options that core_files serves is given."""
    return core_wanted(opt) or density_wanted(opt) or tree_wanted(opt) or presence_wanted(opt)


def _check_alignment_files(opt: argparse.Namespace) -> None:
    """--maf / --variants / --unmapped / --multimaf / --multivariants / --distances / --distancecounts, the four --core options, the four of the density filter and the two trees name files of their own: not each other and not a file the run writes anyway."""
    where = lambda f: os.path.normpath(os.path.join(os.path.abspath(opt.outdir), f))      # noqa: E731
    given = _given(opt, EVERY_FILE_OPTIONS)
    for o, f in given:
        if not f or f.endswith(("/", os.sep)) or os.path.basename(os.path.normpath(f)) in ("", ".", ".."):
            raise PipelineError("%s needs a file name, not '%s'" % (o, f))
    for i, (o, f) in enumerate(given):
        for o2, f2 in given[i + 1:]:
            if where(f) == where(f2):
                raise PipelineError("%s and %s name the same file: %s" % (o, o2, f))
    fixed = ["blocks_coords.txt", "blocks_coords.gff", "genomes_permutations.txt", "coverage_report.txt", "blocks_sequences.fasta"]
    taken = re.compile(r"(blocks_coords\d+\.(txt|gff)|de_bruijn_graph\d*\.dot)$")
    outdir = os.path.abspath(opt.outdir)
    for o, f in given:
        if os.path.dirname(where(f)) == outdir and (os.path.basename(where(f)) in fixed or taken.match(os.path.basename(where(f)))):
            raise PipelineError("%s names a file the program writes itself: %s" % (o, f))


def stages_of(opt: argparse.Namespace) -> List[Tuple[int, int]]:
    return list(PARAMETER_SETS[opt.parameters]) if opt.parameters is not None else read_stage_file(opt.stagefile)


# ------------------------------------------------------------------------------------------ the k rule and the file plan

def stage_trim_k(stages: Sequence[Tuple[int, int]], i: int) -> int:
    """trimK of the per-stage GenerateSyntenyBlocks before stage i: the smallest k so far (src/sibelia.cpp:244)."""
    return min([INT_MAX] + [k for k, _ in stages[:i + 1]])


def final_k(stages: Sequence[Tuple[int, int]], min_block_size: int, lastk: Optional[int] = None) -> Tuple[int, int]:
    """(lastK, trimK) of the final GenerateSyntenyBlocks (src/sibelia.cpp:271-272)."""
    mbs = _as_int(min_block_size)
    trim_k = min([INT_MAX, mbs] + [k for k, _ in stages])
    last_k = lastk if lastk is not None else min(stages[-1][0] if stages else INT_MAX, mbs)
    return last_k, trim_k


def _as_int(u: int) -> int:
    """static_cast<int>(unsigned)"""
    return u - 2 ** 32 if u >= 2 ** 31 else u


def tempdir_of(opt: argparse.Namespace) -> str:
    return opt.tempdir if opt.tempdir is not None else opt.outdir


def stage_graph_written(opt: argparse.Namespace, i: int, outdir_exists: bool) -> bool:
    """de_bruijn_graph<i>.dot of stage i is opened without creating the output directory (src/sibelia.cpp:256-262): it exists only if
    the directory was there already, or if an earlier index created it as its temp directory -- without -r every index does that first
    (src/vertexenumeration.cpp:187), and before stage 0's graph the only index is the one of the stage's blocks."""
    if outdir_exists:
        return True
    if opt.inram or os.path.abspath(tempdir_of(opt)) != os.path.abspath(opt.outdir):
        return False
    return i > 0 or not opt.noblocks


def planned_files(opt: argparse.Namespace, nstages: int, outdir_exists: bool = False) -> List[str]:
    """Names of the files a run with these options writes, relative to the output directory, in the order they are written."""
    out = []
    if (opt.visualize or opt.allstages) and opt.graphfile:
        out += ["de_bruijn_graph%d.dot" % i for i in range(nstages) if stage_graph_written(opt, i, outdir_exists)]
    if not opt.noblocks:
        ext = ".gff" if opt.gff else ".txt"
        out += ["blocks_coords%d%s" % (i, ext) for i in range(nstages + 1)] if opt.allstages else ["blocks_coords" + ext]
        out += ["genomes_permutations.txt", "coverage_report.txt"]
        if opt.sequencesfile:
            out.append("blocks_sequences.fasta")
        out += [f for _, f in _given(opt, EVERY_FILE_OPTIONS)]      # relative names: under the output directory
    if opt.graphfile:
        out.append("de_bruijn_graph%s.dot" % (str(nstages) if opt.allstages else ""))
    return out


class ProgressBar:
    """PutProgressChr (src/util.cpp:89-111): `prev` is a static of the function -- it survives from one bar to the next and is reset
    only when a bar starts."""
    START, RUN, END = 0, 1, 2

    def __init__(self, write: Callable[[str], None]):
        self.prev = 0
        self.write = write

    def __call__(self, progress: int, state: int) -> None:
        while self.prev < progress:
            self.prev += 1
            self.write(".")
        if state == self.START:
            self.prev = 0
            self.write("[")
        elif state == self.END:
            self.write("]\n")


# ------------------------------------------------------------------------------------------ input

def _fasta_error(path: str) -> Optional[str]:
    """The message FASTAReader::GetSequences (src/fasta.cpp:23-104) ends with on this file, None if it parses."""
    valid = b"ACGTURYKMSWBDHWNX-"
    header, have_seq, line = b"", False, 1
    what = None
    with open(path, "rb") as f:
        rows = f.read().split(b"\n")
    if rows and rows[-1] == b"" and len(rows) > 1:
        rows.pop()                                  # text after the last line feed: none
    for raw in rows:
        buf = raw.strip(b" \t\n\v\f\r")
        if not buf:
            continue
        if buf[:1] == b">":
            if header and not have_seq:
                what = "empty sequence"
                break
            if header:
                have_seq = False
            sp = buf.find(b" ")
            header = buf[1:sp] if sp >= 0 else buf[1:]
            if not header:
                what = "empty header"
                break
        else:
            bad = [c for c in buf if bytes([c]).upper() not in valid]
            if bad:
                what = "illegal character: " + chr(bad[0])
                break
            have_seq = True
        line += 1
    if what is None and not have_seq:
        what = "empty sequence"
    return None if what is None else "parse error in %s on line %d: %s" % (path, line, what)


def load_input(filenames: Sequence[str], device: int = -1):
    """-> (finder, names, records in the first file (None for a single file)); the finder carries the record count of every file as
    `file_records` (--multivariants tells the files apart by it).  One file goes through the FASTA loader on the device; several are read on the host and appended to one
    record list, as the reference does (src/sibelia.cpp:209-225)."""
    from . import workloads
    from .api import BlockFinder, SibeliaError
    for f in filenames:
        if not os.path.isfile(f) or not os.access(f, os.R_OK):
            raise PipelineError("Cannot open file " + f)
    try:
        if len(filenames) == 1:
            bf = BlockFinder.from_fasta(filenames[0], device=device)
            bf.file_records = [len(bf.record_names())]
            return bf, None, None
        names, seqs, nfirst, counts = [], [], None, []
        for f in filenames:
            try:
                n, s = workloads.read_fasta(f)
            except ValueError as e:
                raise PipelineError(_fasta_error(f) or "parse error in %s: %s" % (f, e))
            names += n
            seqs += s
            counts.append(len(n))
            if nfirst is None:
                nfirst = len(n)                 # referenceChrId: the records of the first file (src/sibelia.cpp:218-224)
        if sum(len(s) for s in seqs) > MAX_INPUT_SIZE:
            raise PipelineError("Input is larger than 1 GB, can't proceed")
        bf = BlockFinder(seqs, device=device)
        bf.file_records = counts
        return bf, names, nfirst
    except SibeliaError as e:
        text = str(e)
        m = re.search(r"\((.*)\)\s*$", text, re.S)
        if "input exceeds" in text and "total input" in text:
            raise PipelineError("Input is larger than 1 GB, can't proceed")
        raise PipelineError(m.group(1) if m and m.group(1) else text)


def check_duplicate_ids(names: Sequence[str]) -> None:
    """C-Sibelia.py:566-570: the record ids of both files, sorted; the first one that stands twice is an error."""
    ids = sorted(names)
    for a, b in zip(ids, ids[1:]):
        if a == b:
            raise PipelineError('Found duplicated sequence id "%s"' % a)


def first_base(path: str) -> bytes:
    """The first base of the first record of a FASTA file as the file spells it: C-Sibelia.py reads its files itself and does not change
    the case (parse_fasta_file :98-116), and the breakend records quote this base (:451)."""
    import gzip
    with (gzip.open if path.endswith(".gz") else open)(path, "rb") as f:
        seen = False
        for raw in f:
            line = raw.strip()
            if line[:1] == b">":
                if seen:
                    break
                seen = True
            elif line and seen:
                return line[:1]
    return b""


# ------------------------------------------------------------------------------------------ alignments of unique blocks

def skip_limits(opt: argparse.Namespace) -> str:
    """The limits that can leave a block without an alignment: --wideband takes the band width off the list."""
    return "trace memory or length" if opt.wideband else "trace memory, band width or length"


def align_unique_blocks(bf, opt: argparse.Namespace, names: Sequence[str], nfirst: int, complain: Callable[[str], None],
                        history: Optional[Sequence] = None) -> Dict[str, bytes]:
    """--maf / --variants: what C-Sibelia.py does after the reference program has run (src/csibelia/C-Sibelia.py:343-368, :473-484,
    :433-444), with the alignments made on the device (BlockFinder.align_unique_blocks) instead of by one LAGAN process per block.
    Skipped blocks are named through `complain`, one line each, and are absent from both files.  `history`: the block lists of the
    stages and the final one, for --uncovered."""
    from . import formats
    from .api import GALIGN_OK, SibeliaError
    try:
        ids, descs, aligned = bf.align_unique_blocks(opt.minblocksize, nfirst)
    except SibeliaError as e:
        raise PipelineError(str(e))
    size = bf.record_sizes()
    groups, records = [], []
    for block, (ca, sa, ea, ra, cb, sb, eb, rb), al in zip(ids, descs, aligned):
        if al.status != GALIGN_OK:
            complain("block %d not aligned: %s:%d-%d against %s:%d-%d is beyond the limits of one alignment "
                     "(%s, DESIGN.md 0.2)\n" % (block, names[ca], sa + 1, ea, names[cb], sb + 1, eb, skip_limits(opt)))
            continue
        groups.append([formats.maf_line(names[ca], sa, ea, ra, size[ca], al.row_a), formats.maf_line(names[cb], sb, eb, rb, size[cb], al.row_b)])
        if opt.variants is not None:
            records += [(names[ca],) + v for v in formats.variants_from_runs(al.runs, al.row_a, al.row_b, sa, ea, ra)]
    out = {}
    if opt.maf is not None:
        out[opt.maf] = formats.maf_text(groups, opt.gapopen)
    if opt.variants is not None and opt.uncovered:
        out.update(uncovered_files(bf, opt, names, nfirst, records, history))
    elif opt.variants is not None:
        out[opt.variants] = formats.vcf_text(names[0], records, opt.gapopen)
    return out


def uncovered_files(bf, opt: argparse.Namespace, names: Sequence[str], nfirst: int, records, history: Sequence) -> Dict[str, bytes]:
    """--uncovered / --unmapped: C-Sibelia.py's calls from the regions no mixed block of any stage covers (:373-427) next
    to the alignment `records` in the VCF (:575-585), and the insertions it cannot place as breakend records or, with --unmapped, as
    FASTA (:493-500).  The runs come from interval bookkeeping in the library (BlockFinder.uncovered_calls); each file is one piece
    list whose record ranges -- the alleles -- are spelled on the device (BlockFinder.spell_text)."""
    from . import formats
    from .api import SibeliaError
    try:
        calls = bf.uncovered_calls(history, opt.minblocksize, nfirst)
        vcf = formats.vcf_pieces(names, bf.record_sizes()[0], first_base(opt.filenames[0]), records, calls, opt.unmapped is None, opt.gapopen)
        out = {opt.variants: bf.spell_text(vcf.pieces(), vcf.literals)}
        if opt.unmapped is not None:
            fa = formats.unmapped_fasta_pieces(names, calls)
            out[opt.unmapped] = bf.spell_text(fa.pieces(), fa.literals)
    except SibeliaError as e:
        raise PipelineError(str(e))
    return out


def _file_of_record(file_records: Sequence[int]) -> Callable[[int], int]:
    import bisect
    first = [0]
    for n in file_records:
        first.append(first[-1] + n)
    return lambda c: bisect.bisect_right(first, int(c)) - 1


def _instances_by_id(blocks, file_records: Sequence[int]) -> List[Tuple[int, List[Tuple[int, int]]]]:
    """(id, [(file, length) per instance]) of a block list (formats.BLOCK_DTYPE), in ascending id."""
    file_of = _file_of_record(file_records)
    by_id: Dict[int, List[Tuple[int, int]]] = {}
    for b in blocks:
        by_id.setdefault(abs(int(b["id"])), []).append((file_of(b["chr"]), int(b["end"]) - int(b["start"])))
    return sorted(by_id.items())


def _once_per_file(inst: Sequence[Tuple[int, int]], min_block_size: int) -> bool:
    """Every instance is at least min_block_size long and at most one lies on the records of each file."""
    files = [f for f, _ in inst]
    return all(n >= min_block_size for _, n in inst) and len(set(files)) == len(files)


def qualifying_blocks(blocks, file_records: Sequence[int], min_block_size: int) -> List[int]:
    """The ids --multivariants calls from, on a block list (formats.BLOCK_DTYPE): EVERY instance of the id is at least min_block_size
    long, there are at least two, exactly one lies on the records of the first file and at most one on those of each other file.  For
    two files this is determine_unique_block (C-Sibelia.py:314-323)."""
    return [block for block, inst in _instances_by_id(blocks, file_records)
            if len(inst) >= 2 and _once_per_file(inst, min_block_size) and [f for f, _ in inst].count(0) == 1]


def distance_blocks(blocks, file_records: Sequence[int], min_block_size: int) -> List[int]:
    """The ids --distances / --distancecounts count over, on a block list (formats.BLOCK_DTYPE): there are at least two instances of
    the id, EVERY one is at least min_block_size long, and at most one lies on the records of each file.  Unlike qualifying_blocks it
    does not ask for an instance in the first file."""
    return [block for block, inst in _instances_by_id(blocks, file_records) if len(inst) >= 2 and _once_per_file(inst, min_block_size)]


def core_blocks(blocks, file_records: Sequence[int], min_block_size: int) -> List[int]:
    """The ids of the core blocks of a block list (formats.BLOCK_DTYPE), what the four --core options concatenate: the id has exactly
    one instance on the records of EACH input file -- as many instances as there are files -- and every one is at least min_block_size
    long.  The subset of distance_blocks that reaches every file; for two files the two are the same."""
    return [block for block, inst in _instances_by_id(blocks, file_records)
            if all(n >= min_block_size for _, n in inst) and sorted(f for f, _ in inst) == list(range(len(file_records)))]


def soft_core_blocks(blocks, file_records: Sequence[int], min_block_size: int, coremin: int) -> List[int]:
    """The ids of the soft-core blocks of a block list (formats.BLOCK_DTYPE), what the --core options concatenate under --coremin: every
    instance of the id is at least min_block_size long, exactly one lies on the records of the first file, at most one on those of each
    other file, and they lie in at least `coremin` files -- qualifying_blocks with a floor on the number of files, so the first file's
    instance stays the centre.  With coremin the number of files these are core_blocks."""
    return [block for block, inst in _instances_by_id(blocks, file_records)
            if len(inst) >= max(coremin, 1) and _once_per_file(inst, min_block_size) and [f for f, _ in inst].count(0) == 1]


def core_files(bf, opt: argparse.Namespace, names: Sequence[str], ids: Sequence[int], insts, aligned, core, complain: Callable[[str], None]) -> Dict[str, bytes]:
    """--corealignment / --corepartitions / --coresnps / --coresites from the alignments of one align_block_groups call: the class of an
    instance is the file of its record, the wanted groups are the aligned blocks of `core` (core_blocks); the rows are concatenated and
    filtered on the device (BlockFinder.group_concat), one call per mode.  The first file's instance of a core block
    sorts first, so it is the centre: the positions of --coresites are read on it.
    --corefiltered / --corefilteredsnps / --corefilteredsites / --coredense, after those: the density mask of the same wanted groups
    against their centre -- the first file -- on the device (BlockFinder.group_mask), then the same two concatenations
    of the masked rows (set_masked); in a core block row i is file i's.
    --coretree / --corefilteredtree: one BlockFinder.group_bootstrap call each on the rows / the masked rows and the
    tree of its counts (tree.py); a tree that cannot be built is named through `complain` and its file is absent from the result.
    --coreconsensus / --coreboottrees and --corefilteredconsensus / --corefilteredboottrees: from the same call as the tree of their rows,
    whose B + 1 matrices go through one BlockFinder.nj_batch call (tree.tree_files); absent with their tree.
    --coremin below the number of files: `core` holds soft_core_blocks, all of the above runs inside a set_partial
    section, the tables get their `# coremin=M` line and the trees divide by group_bootstrap_pairs, the clean columns per pair of files.
    --corepresence: which files every wanted and aligned block has an instance in, from `cls`.
    --corebranches / --corebranchsites / --coresnptree and their filtered twins: after the tree of their rows, from the same group_bootstrap
    call and its main tree, one BlockFinder.group_parsimony call; absent with their tree."""
    from . import formats, tree
    from .api import CONCAT_ALL, CONCAT_VARIABLE, GALIGN_OK, SibeliaError
    file_of = _file_of_record(bf.file_records)
    n = len(bf.file_records)
    cls = [file_of(c) for inst in insts for c, _, _, _ in inst]
    want = [block in core and al.status == GALIGN_OK for block, al in zip(ids, aligned)]
    flat = [0]                                          # the first instance of every group in cls
    for inst in insts:
        flat.append(flat[-1] + len(inst))
    soft = opt.coremin < n                              # the soft core: partial groups on the device, comment lines in the files
    coremin = opt.coremin if soft else 0
    if not any(want):
        if soft:
            complain("no core block: no block has exactly one instance of at least %d bases in the first input file, at most one in each other "
                     "and instances in at least %d input files (--coremin %d), and was aligned\n" % (opt.minblocksize, opt.coremin, opt.coremin))
        else:
            complain("no core block: no block has exactly one instance of at least %d bases in every input file and was aligned\n" % opt.minblocksize)
    headers = [b">" + a.encode("latin1") + b"\n" for a in file_names(opt.filenames)]
    out = {}

    def tree_files(masked: bool):
        """the tree, the consensus and the replicate trees wanted of the rows (masked: of the masked rows): one group_bootstrap call, and
        in tree.tree_files one nj_batch call -- a finder without one (more than 64 files go the same way) has its trees joined there"""
        kinds = ("tree", "consensus", "boottrees")     # the texts of tree.tree_files, in its order
        given = [(kind, o, getattr(opt, a)) for kind, (o, a) in zip(kinds, ROWS_TREE_OPTIONS[masked]) if getattr(opt, a) is not None]
        mapped = [(kind, o, getattr(opt, a)) for kind, (o, a) in zip(("branches", "branchsites", "snptree"), ROWS_BRANCH_OPTIONS[masked]) if getattr(opt, a) is not None]
        if not (given or mapped) or not any(want):      # no core block: said above
            return
        counts, nsites, nclean = bf.group_bootstrap(cls, n, opt.bootstrap, opt.bootseed, 0, want)
        why = "no variable column in the core-genome alignment" if nsites == 0 else None
        keep = {}
        if why is None:
            try:
                texts = tree.tree_files(counts, bf.group_bootstrap_pairs() if soft else nclean, opt.treemodel, file_names(opt.filenames), getattr(bf, "nj_batch", None),
                                        [kind for kind, _, _ in given] + (["tree"] if mapped else []), keep)
            except (tree.Saturated, tree.NoSharedColumn) as e:
                why = str(e)
        if why is not None:
            for _, o, _ in given + mapped:
                complain("%s not written: %s\n" % (o, why))
            return
        for kind, _, f in given:
            out[f] = texts[kinds.index(kind)].encode("latin1")
        if mapped:
            branch_files(keep["tree"], keep["support"], site_rows.get(masked), mapped)

    def branch_files(main, held, rows, mapped):
        """the branch table, the change table and the SNP-scaled tree of the main tree: one BlockFinder.group_parsimony
        call on the sites the group_bootstrap call before it left packed on the device, with the edges of the tree that call's counts gave"""
        ecounts, steps, least, changes = bf.group_parsimony([(u, v) for u, v, _ in main.edges])
        order = tree.branches(main)
        files = file_names(opt.filenames)
        number = {e: k + 1 for k, (_, e, _, _) in enumerate(order)}
        steps, least = steps.tolist(), least.tolist()
        for kind, _, f in mapped:
            if kind == "branches":
                out[f] = formats.core_branches_text(
                    [([files[x] for x in range(n) if mask >> x & 1], length, tree.support_label(held.get(mask, 0), opt.bootstrap) if held is not None and v >= n else None,
                      ecounts[e].tolist()) for v, e, mask, length in order], steps, least, opt.gapopen, coremin)
            elif kind == "branchsites":
                found = sorted(zip(changes["site"].tolist(), [number[e] for e in changes["edge"].tolist()], changes["from"].tolist(), changes["to"].tolist()))
                out[f] = formats.core_branch_sites_text(rows, found, steps, least, opt.gapopen, coremin)
            else:
                out[f] = tree.newick(main, files, held, opt.bootstrap, {v: int(ecounts[e].sum()) for v, e, _, _ in order}).encode("latin1")

    def site_rows_of(sites):
        return [(ids[g], names[insts[g][0][0]]) + tuple(insts[g][0][1:]) + (before,) for g, _, before in sites]
    site_rows = {}                                      # masked -> the rows of formats.core_sites_text of that kind of rows
    try:
        if soft:
            bf.set_partial(True)
        if opt.corepresence is not None:
            out[opt.corepresence] = formats.core_presence_text(
                file_names(opt.filenames), [(ids[g], [f in cls[flat[g]:flat[g + 1]] for f in range(n)]) for g in range(len(ids)) if want[g] and aligned[g].L], opt.gapopen, coremin)
        if opt.corealignment is not None or opt.corepartitions is not None:
            text, parts, _ = bf.group_concat(cls, n, headers, CONCAT_ALL, formats.CORE_WIDTH, want)
            if opt.corealignment is not None:
                out[opt.corealignment] = text
            if opt.corepartitions is not None:
                out[opt.corepartitions] = formats.core_partitions_text([(ids[g], first, ncols) for g, first, ncols in parts], opt.gapopen, coremin)
        if opt.coresnps is not None or opt.coresites is not None or opt.corebranchsites is not None:
            text, _, sites = bf.group_concat(cls, n, headers, CONCAT_VARIABLE, formats.CORE_WIDTH, want)
            site_rows[False] = site_rows_of(sites)
            if opt.coresnps is not None:
                out[opt.coresnps] = text
            if opt.coresites is not None:
                out[opt.coresites] = formats.core_sites_text(site_rows[False], opt.gapopen, coremin)
        tree_files(False)
        if density_wanted(opt):
            intervals = bf.group_mask(opt.densitywindow, opt.densitymax, want)
            bf.set_masked(True)
            try:
                if opt.corefiltered is not None:
                    out[opt.corefiltered] = bf.group_concat(cls, n, headers, CONCAT_ALL, formats.CORE_WIDTH, want)[0]
                if opt.corefilteredsnps is not None or opt.corefilteredsites is not None or opt.corefilteredbranchsites is not None:
                    text, _, sites = bf.group_concat(cls, n, headers, CONCAT_VARIABLE, formats.CORE_WIDTH, want)
                    site_rows[True] = site_rows_of(sites)
                    if opt.corefilteredsnps is not None:
                        out[opt.corefilteredsnps] = text
                    if opt.corefilteredsites is not None:
                        out[opt.corefilteredsites] = formats.core_sites_text(site_rows[True], opt.gapopen, coremin)
                tree_files(True)
            finally:
                bf.set_masked(False)
            if opt.coredense is not None:
                first, at = {}, 0                       # the first column of every wanted group in the concatenation: the parts of mode ALL
                for g, al in enumerate(aligned):
                    if want[g] and al.L:
                        first[g], at = at, at + al.L
                files = file_names(opt.filenames)
                out[opt.coredense] = formats.core_dense_text(
                    [(files[cls[flat[g] + row]], ids[g], names[insts[g][0][0]]) + tuple(insts[g][0][1:]) + (before_lo, before_hi, ndiff, first[g] + lo, first[g] + hi)
                     for g, row, lo, hi, before_lo, before_hi, ndiff in intervals], opt.densitywindow, opt.densitymax, opt.gapopen, coremin)
    except SibeliaError as e:
        raise PipelineError(str(e))
    finally:
        if soft:
            bf.set_partial(False)
    made = {f: out[f] for _, f in _given(opt, CORE_OPTIONS + DENSITY_OPTIONS + PRESENCE_OPTIONS)}
    made.update({f: out[f] for _, f in _given(opt, ALL_TREE_OPTIONS) if f in out})      # a tree that could not be built was named and is absent
    return made


def distance_files(bf, opt: argparse.Namespace, ids: Sequence[int], insts, aligned, used, complain: Callable[[str], None]) -> Dict[str, bytes]:
    """--distances / --distancecounts from the alignments of one align_block_groups call: the class of an instance is the file of its
    record, the wanted groups are the blocks `used` (distance_blocks); the row comparisons run on the device
    (BlockFinder.group_distances) and blocks(f, g) -- the used and aligned blocks with an instance in both files -- is
    counted here."""
    from . import formats
    from .api import GALIGN_OK, SibeliaError
    file_of = _file_of_record(bf.file_records)
    n = len(bf.file_records)
    try:
        counts = bf.group_distances([file_of(c) for inst in insts for c, _, _, _ in inst], n, [block in used for block in ids])
    except SibeliaError as e:
        raise PipelineError(str(e))
    shared = [[0] * n for _ in range(n)]
    for block, inst, al in zip(ids, insts, aligned):
        if block in used and al.status == GALIGN_OK:
            files = sorted({file_of(c) for c, _, _, _ in inst})
            for f in files:
                for g in files:
                    shared[f][g] += f != g
    names = file_names(opt.filenames)
    out = {}
    if opt.distances is not None:
        out[opt.distances] = formats.distances_text(names, counts, complain)
    if opt.distancecounts is not None:
        out[opt.distancecounts] = formats.distance_counts_text(names, counts, shared, opt.gapopen)
    return out


def align_block_groups(bf, opt: argparse.Namespace, names: Sequence[str], complain: Callable[[str], None], blocks=None) -> Dict[str, bytes]:
    """--multimaf: one MAF paragraph per block with at least two instances, in ascending id, its `s` lines in the order of the alignment
    (centre first: BlockFinder.align_block_groups).  A skipped block is named through `complain` in one line and is absent.
    --multivariants: the calls read off the SAME alignments (one align_block_groups call serves both; BlockFinder.group_variants,
    DESIGN.md 0.6) for the qualifying blocks of the final list `blocks` (qualifying_blocks) as a multi-sample VCF; the first-file
    instance sorts first, so it is the centre and its alleles are REF.
    --distances / --distancecounts: the pairwise counts of the same alignments (distance_files), written after the two.
    --corealignment / --corepartitions / --coresnps / --coresites: the concatenation of the same alignments (core_files), after those;
    --corefiltered / --corefilteredsnps / --corefilteredsites / --coredense: the same of their masked rows (core_files);
    --coretree / --corefilteredtree: the trees of the two (core_files); the consensus and the replicate trees of the two, last."""
    from . import formats
    from .api import GALIGN_OK, SibeliaError
    try:
        ids, insts, aligned = bf.align_block_groups(opt.minblocksize)
    except SibeliaError as e:
        raise PipelineError(str(e))
    size = bf.record_sizes()
    qualify = set(qualifying_blocks(blocks, bf.file_records, opt.minblocksize)) if opt.multivariants is not None else set()
    distances = opt.distances is not None or opt.distancecounts is not None
    used = set(distance_blocks(blocks, bf.file_records, opt.minblocksize)) if distances else set()
    core = set()
    if concat_wanted(opt):
        soft = opt.coremin < len(bf.file_records)
        core = set(soft_core_blocks(blocks, bf.file_records, opt.minblocksize, opt.coremin) if soft else core_blocks(blocks, bf.file_records, opt.minblocksize))
    groups = []
    for block, inst, al in zip(ids, insts, aligned):
        if al.status != GALIGN_OK:
            if opt.multimaf is not None or block in qualify or block in used or block in core:
                complain("block %d not aligned: one of its %d instances against %s:%d-%d is beyond the limits of one alignment "
                         "(%s, DESIGN.md 0.2)\n" % (block, len(inst), names[inst[0][0]], inst[0][1] + 1, inst[0][2], skip_limits(opt)))
            continue
        if opt.multimaf is not None:
            groups.append([formats.maf_line(names[c], s, e, rev, size[c], row) for (c, s, e, rev), row in zip(inst, al.rows)])
    out = {}
    if opt.multimaf is not None:
        out[opt.multimaf] = formats.maf_text(groups, opt.gapopen)
    if opt.multivariants is not None:
        try:
            segments = bf.group_variants([block in qualify for block in ids])
        except SibeliaError as e:
            raise PipelineError(str(e))
        file_of = _file_of_record(bf.file_records)
        by_group: Dict[int, list] = {}
        for seg in segments:
            by_group.setdefault(seg[0], []).append(seg)
        records = []
        for g, segs in sorted(by_group.items()):
            inst = insts[g]
            row_of = {file_of(c): i for i, (c, _, _, _) in enumerate(inst)}      # file -> row (at most one each)
            c0, s0, e0, rev0 = inst[0]
            for pos, alleles in formats.group_variants_records(segs, s0, e0, rev0):
                records.append((names[c0], pos, ids[g], alleles[0],
                                [alleles[row_of[f]] if f in row_of else None for f in range(1, len(bf.file_records))]))
        out[opt.multivariants] = formats.multi_vcf_text(names[0], sample_names(opt.filenames), records, opt.gapopen)
    if distances:
        out.update(distance_files(bf, opt, ids, insts, aligned, used, complain))
    if concat_wanted(opt):
        out.update(core_files(bf, opt, names, ids, insts, aligned, core, complain))
    return out


# ------------------------------------------------------------------------------------------ main

def run(argv: Sequence[str], write: Optional[Callable[[str], None]] = None, outdir_exists: Optional[bool] = None) -> Tuple[int, Dict[str, bytes], str]:
    """The reference's main (src/sibelia.cpp:186-345).  `write` receives the standard output as it is produced; `outdir_exists`
    (default: look) is whether the output directory is there before the run.  Raises PipelineError for what main reports as an error."""
    from . import formats
    from .api import SibeliaError, glue_stripes
    opt = parse_args(argv)
    stages = stages_of(opt)
    if outdir_exists is None:
        outdir_exists = os.path.isdir(opt.outdir)
    printed: List[str] = []

    def say(s: str) -> None:
        printed.append(s)
        if write:
            write(s)

    bar = ProgressBar(say)
    bf, names, nfirst = load_input(opt.filenames, opt.device)
    files: Dict[str, bytes] = {}
    try:
        if opt.uncovered:
            check_duplicate_ids(names)
        if not opt.inram:
            bf.set_tempfile_mode(True)            # BlockFinder(chrList, tempDir): temp-file names come out of the same rand() stream
        nchr = len(names) if names is not None else len(bf.record_names())
        history = [None] * (len(stages) + 1)
        every_stage = opt.visualize or opt.allstages
        for i, (k, branch) in enumerate(stages):
            if every_stage:
                if not opt.noblocks:
                    b = bf.GenerateSyntenyBlocks(k, stage_trim_k(stages, i), k, opt.sharedonly)
                    history[i] = b if opt.nopostprocess else glue_stripes(b, nchr)
                if opt.graphfile:
                    text = formats.dot_text(bf.list_edges(k))      # runs whether the file can be opened or not: it draws from rand()
                    if stage_graph_written(opt, i, outdir_exists):
                        files["de_bruijn_graph%d.dot" % i] = text
            say("Simplification stage %d of %d\n" % (i + 1, len(stages)))
            say("Enumerating vertices of the graph, then performing bulge removal...\n")
            bf.PerformGraphSimplifications(k, branch, opt.maxiterations, bar)
        say("Finding synteny blocks and generating the output...\n")
        last_k, trim_k = final_k(stages, opt.minblocksize, opt.lastk)
        if not opt.noblocks:
            bf.GenerateSyntenyBlocks(last_k, trim_k, opt.minblocksize, opt.sharedonly)
            blocks, (coords, perms, coverage) = bf.postprocess(names, glue=not opt.nopostprocess)
            if opt.correctboundaries:           # Postprocessor::ImproveBlockBoundaries (src/sibelia.cpp:295-298), before any writer
                try:
                    blocks, (coords, perms, coverage) = bf.correct_boundaries(opt.minblocksize, nfirst, names)
                except SibeliaError as e:
                    raise PipelineError(str(e))
            history[-1] = blocks
            writer, ext = (bf.blocks_gff, ".gff") if opt.gff else (bf.blocks_coords, ".txt")
            if opt.allstages:
                for i, h in enumerate(history):
                    files["blocks_coords%d%s" % (i, ext)] = writer(h, names)
            else:
                files["blocks_coords" + ext] = writer(None, names) if opt.gff else coords
            files["genomes_permutations.txt"] = perms
            files["coverage_report.txt"] = coverage
            if opt.sequencesfile:
                files["blocks_sequences.fasta"] = bf.blocks_sequences(None, names)
            if opt.gapopen:                       # after the boundary correction, which keeps the reference's own alignment
                bf.set_gap_open(opt.gapopen)
            if opt.wideband:
                bf.set_wide(True)
            if opt.maf is not None or opt.variants is not None:      # on the final list: after the boundary correction, if that ran
                files.update(align_unique_blocks(bf, opt, names, nfirst, sys.stderr.write, history))
            if _given(opt, GROUP_OPTIONS + BRANCH_OPTIONS):          # likewise on the final list
                files.update(align_block_groups(bf, opt, names if names is not None else bf.record_names(), sys.stderr.write, blocks))
        if opt.graphfile:
            files["de_bruijn_graph%s.dot" % (str(len(stages)) if opt.allstages else "")] = formats.dot_text(bf.list_edges(last_k))
    finally:
        bf.close()
    unbuilt = [f for _, f in _given(opt, ALL_TREE_OPTIONS) if f not in files]      # a tree that could not be built was named on standard error
    assert list(files) == [f for f in planned_files(opt, len(stages), outdir_exists) if f not in unbuilt]
    return 0, files, "".join(printed)


def write_files(outdir: str, files: Dict[str, bytes]) -> None:
    """Writes what `run` returned under the output directory; a name with a directory part (--maf sub/a.maf) gets that directory."""
    os.makedirs(outdir, exist_ok=True)
    for name, data in files.items():
        path = os.path.join(outdir, name)
        os.makedirs(os.path.dirname(path) or ".", exist_ok=True)
        with open(path, "wb") as f:
            f.write(data)


def main(argv: Optional[Sequence[str]] = None) -> int:
    argv = sys.argv[1:] if argv is None else list(argv)

    def write(s: str) -> None:
        sys.stdout.write(s)
        sys.stdout.flush()
    try:
        opt = parse_args(argv)
        rc, files, _ = run(argv, write=write, outdir_exists=os.path.isdir(opt.outdir))
        if not opt.inram:                           # the reference's indices create their temp directory (by default the output directory)
            os.makedirs(tempdir_of(opt), exist_ok=True)
        write_files(opt.outdir, files)
        return rc
    except PipelineError as e:
        sys.stderr.write("error: %s\n" % e)
        return 1
