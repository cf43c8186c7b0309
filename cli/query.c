/*
 * query.c -- deBWT-query: exact pattern search over a BWT that deBWT wrote (OUT, OUT.#, OUT.$), through the FM-index of
 * libdebwt_hip.so (debwt_fm_*).
 *
 *   deBWT-query index  -i OUT [-t T] [--iupac SEED] [--device D] [--sa S] INPUT.fa[.gz]
 *   deBWT-query count  -i OUT [--device D] [--mismatches K] [--both-strands] [--best] [--records] PATTERNS.fa|.fq
 *   deBWT-query locate -i OUT [--device D] [--max-hits M] [--mismatches K] [--both-strands] [--best] PATTERNS.fa|.fq
 *   deBWT-query mems   -i OUT [--device D] [--min-len L] [--both-strands] [--max-hits M] READS.fa|.fq
 *   deBWT-query overlaps -i OUT [--device D] [--min-overlap L] [--both-strands] [--longest] [--no-self]
 *                      [--max-mismatches K [--max-error-permille R]] READS.fa|.fq
 *   deBWT-query map    -i OUT [--ref INPUT.fa[.gz] [-t T] [--iupac SEED]] [--device D] [--min-len L] [--band W]
 *                      [--max-occ N] [--min-score S] [--chain [--max-gap G]]
 *                      [--mate READS2.fa|.fq [--insert LO,HI] [--no-rescue]] READS.fa|.fq
 *   deBWT-query extract -i OUT [--device D] --all | REGIONS.txt
 *   deBWT-query kmers  -i OUT -k K [--device D] [--both-strands] READS.fa|.fq
 *   deBWT-query correct -i OUT -k K [--device D] [--min-count T|auto] [--rounds R] [--forward] [--report FILE] READS.fa|.fq
 *   deBWT-query spectrum -i OUT -k K [--device D] [--forward] [--bins N] [--list FILE [--at-least A] [--at-most B]]
 *   deBWT-query lcp    -i OUT [--device D] [--max-lcp C] [--lcp FILE] [--sa FILE] [--da FILE] [--profile K]
 *   deBWT-query graph  -i OUT [--device D] [--min-overlap L] [--all-edges] [--both-strands] [--states FILE]
 *                      [--clean] [--max-tip N] [--max-bubble N] [--clean-rounds R]
 *   deBWT-query unitigs -i OUT [--device D] [--min-overlap L] [--both-strands] [--states FILE]
 *                      [--clean] [--max-tip N] [--max-bubble N] [--clean-rounds R]
 *
 * index ingests INPUT as deBWT does (same -t, same --iupac SEED: the same text), checks that OUT is that text's BWT while
 * it samples the suffix array every S rows (a power of two in 1..1024, default 32), and writes OUT.sa; exit status 1 when
 * OUT is not INPUT's BWT.  count and locate need OUT, OUT.#, OUT.$ and OUT.sa only.  They print one TSV line per pattern:
 * name, occurrences and (locate) the occurrences as record:offset, ascending -- records are 0-based in file order.
 * --max-hits M lists the first M occurrences in suffix order (the count column stays the full count).  A pattern with a
 * letter outside ACGTacgt occurs 0 times.
 *
 * --mismatches K (0..4), --both-strands and --best search with debwt_fm_search: occurrences of strings within Hamming
 * distance K of the pattern (a letter outside ACGTacgt matches no base), also of its reverse complement, only those of
 * the smallest distance found.  With any of them, count prints name, total and the occurrences per distance c0,..,cK;
 * locate prints name, total and record:offset:strand:mismatches (strand + or -), ascending by (record, offset, strand),
 * the first M of them with --max-hits M.
 *
 * mems prints the maximal exact matches of at least L bases (default 19, BWA-MEM's -k; debwt_fm_mems) of every read, and
 * with --both-strands those of its reverse complement: one line per MEM, name, strand (+ or -), qbeg, qend (0-based, end
 * exclusive, in the read's own coordinates on both strands), occurrences and record:offset ascending.  --max-hits M lists
 * the first M occurrences in suffix order (the count column stays the full count).  Reads without MEMs print nothing.
 *
 * overlaps prints the suffix-prefix overlaps of every read with the records of OUT (debwt_fm_overlaps): one line per
 * (record, length) of at least L bases (default 20) such that the record begins with the read's last `length` bases --
 * name, strand (+ or -), record, length and flags: C when the whole record is the overlap, W when the whole read is, CW,
 * or "." -- ordered by (strand, length descending, record).  --both-strands adds the overlaps of the read's reverse
 * complement (strand -: the record begins with the reverse complement of the read's first `length` bases); --longest
 * keeps the longest overlap per read, strand and record; --no-self, for querying the indexed file itself, drops read
 * number i's overlap with record i over its whole length.  It needs OUT, OUT.#, OUT.$ and OUT.sa only.
 * --max-mismatches K (0..4) goes through debwt_fm_overlaps_mm instead: the record's first `length` bases may differ from
 * the read's last `length` in up to K columns (a letter outside ACGTacgt is a mismatch), and with --max-error-permille R
 * (0..1000, only with --max-mismatches) in at most R / 1000 of the columns; every line then gets a sixth column, the
 * mismatches of that overlap (also with K = 0).  Without --max-mismatches the output is what it was.  Reads hold at most
 * 1024 bases there.
 *
 * map aligns every read (debwt_fm_map: MEM seeds of at least L bases, at most N occurrences of each, clustered by diagonal,
 * banded affine-gap extension with half-width W, 0..63; a plain heuristic, not BWA-MEM's).  The index holds no text:
 * without --ref it is restored on the GPU from OUT, OUT.#, OUT.$ and OUT.sa alone (debwt_fm_restore_text; a note on
 * stderr says so); with --ref the input is named again, packed as index packs it (same -t, same --iupac SEED) and
 * refused when it is not the text of OUT.  Both give the same PAF.  One PAF line per mapped read: name, length, query start and end (on the read's own strand), strand,
 * record number, record length, target start and end, matching bases, alignment columns, mapping quality, then AS:i:
 * (score), NM:i: (mismatches + gap bases) and cg:Z: (CIGAR along the text).  Reads that are not mapped print nothing.
 * --chain maps with debwt_fm_map_chained instead: the seeds of a read are chained across diagonals (steps of at most W,
 * stretches of at most G bases between two seeds, default 5000) and the band follows the chain, so a read whose indels
 * add up to more than W is still aligned end to end.  The PAF columns are the same.
 * --mate READS2 maps paired ends with debwt_fm_map_pairs: read i of READS and read i of READS2 are the mates of pair i (the
 * files must hold the same number of reads; not with --chain).  --insert LO,HI gives the bounds of the template length
 * (LO <= HI <= 16384) instead of estimating them from the pairs that map uniquely; --no-rescue keeps a mate without a
 * seed unmapped instead of aligning it in the window its partner leaves it.  Output: mate 1's line, then mate 2's, for
 * every pair, mapped mates only, with three more tags: pr:A:P on both mates of a proper pair and pr:A:U otherwise, tl:i:
 * (the template length, positive on the forward mate and negative on the reverse one; proper pairs only) and rs:i:1 on a
 * mate that was placed by the rescue.
 *
 * extract gives the indexed sequence back as FASTA (debwt_fm_extract); it needs OUT, OUT.#, OUT.$ and OUT.sa only.  --all
 * writes every record, header >J (the 0-based record number the other subcommands print), the sequence on one line, in
 * upper case (the index holds four codes: neither the case nor the IUPAC letters nor the names of the input).
 * REGIONS.txt holds one region per line, J (a whole record) or J:BEG-END (0-based, end exclusive: the coordinates locate
 * prints); the header is the region as given.  A malformed line or a region outside its record: exit status 1 with a
 * message naming the line, and nothing on stdout.  The output is produced in batches of about 64 MB.
 *
 * kmers prints the count of every K-mer along every read (debwt_fm_kmer_counts): one line per read, name, TAB, the counts
 * of the K-mers at positions 0, 1, .. joined by commas, or * when the read is shorter than K.  A K-mer with a letter
 * outside ACGTacgt counts 0; --both-strands adds the occurrences of the reverse complement.
 *
 * correct removes substitution errors from the reads with the K-mer counts of the indexed collection (debwt_fm_correct;
 * a K-mer is weak below T occurrences, default 3, at most R rounds, 1..16, default 4, both strands unless --forward) and
 * writes them as FASTA to stdout, the names unchanged, one line per sequence; a fixed base is in upper case, every other
 * letter as it came.  --report FILE writes a TSV of name, status (short, clean, fixed or weak), fixes, weak_before and
 * weak_after; stderr gets one summary line.  Both need OUT, OUT.#, OUT.$ and OUT.sa only, and -k is required.
 * --min-count auto takes T from the K-mer spectrum of the collection (its valley, see spectrum; same K, same strands, 256
 * bins), names it on stderr and exits 1 with a message when the spectrum has no valley.
 *
 * spectrum prints the K-mer spectrum of the indexed collection (debwt_fm_spectrum; K in 1..32, both strands unless
 * --forward: a K-mer and its reverse complement are one K-mer under the smaller of the two, and one that is its own
 * reverse complement counts twice, as in kmers --both-strands).  No reads are needed: every distinct K-mer is met once by
 * a walk over the index.  stdout: the lines "# k", "# strands", "# distinct", "# total", "# valley", "# peak" and
 * "# est_size" (name, TAB, value), then mult<TAB>distinct for every non-empty bin of the histogram of N bins (2..4096,
 * default 256); the last bin holds N - 1 and above and is printed as >=N-1.  valley is the first multiplicity whose
 * successor has more K-mers (K-mers below it are weak), peak the fullest bin behind it, est_size the K-mers from the
 * valley on divided by the peak; all three are 0 when the histogram only falls.  --list FILE gets KMER<TAB>mult for every
 * distinct K-mer of multiplicity A (--at-least, default 1) to B (--at-most, default 2^32 - 1), in the order of the
 * K-mers (debwt_fm_kmer_list).  It needs OUT, OUT.#, OUT.$ and OUT.sa only and takes no file argument.
 *
 * lcp builds the suffix array, the LCP array and the record array of the indexed collection on the GPU
 * (debwt_fm_esa_build, Definition 10 of debwt_hip.h): lcp[r] is the common prefix of the suffixes of rows r - 1 and r of
 * OUT, cut at the first separator of either, stored as min(lcp, C) with --max-lcp C (default: no cap).  --lcp FILE, --sa
 * FILE and --da FILE get the arrays as raw little-endian files of n entries: u32 LCP values, u64 text positions, u32
 * record numbers.  stdout: one line "# n=N max=M max_row=R prev=J:OFF pos=J:OFF mean=X" (TAB-separated; M the largest
 * stored value, R the first row that holds it, prev and pos the places of the suffixes of rows R - 1 and R as
 * record:offset -- the longest repeat -- and X the mean of the stored values with six decimals); with --profile K (1..4096,
 * at most C) K lines k<TAB>distinct follow, the number of distinct strings of k bases inside records for k = 1..K.  It
 * needs OUT, OUT.#, OUT.$ and OUT.sa only (the text is restored on the GPU) and takes no file argument.
 *
 * repeats lists the repeats of the indexed collection from the LCP array (debwt_fm_repeats, Definition 11 of debwt_hip.h):
 * the maximal repeats of at least L bases (--min-len, default 20) with A (--min-occ, default 2) to B (--max-occ, default
 * no bound) occurrences inside records; --supermaximal lists the supermaximal ones, --intervals every interval of the LCP
 * array, left-diverse or not.  It builds the arrays with the suffix array kept; with --max-lcp C the LCP values are capped
 * at C and only repeats shorter than C are listed (L must be below C).  stdout: one line "# intervals=I maximal=M
 * supermaximal=S reported=R longest=LEN" (TAB-separated; I, M and S count the intervals of at least L bases before the
 * occurrence bounds and the kind are applied), then one line per repeat in the library's order: len, occ, S (supermaximal), M
 * (maximal) or - (an interval that is not left-diverse), the occurrences behind A,C,G,T and at a record's start
 * (a,c,g,t,s), and the first occurrence in row order as record:offset, TAB-separated.  --seq appends the string (read
 * through debwt_fm_extract), --occurrences every occurrence as record:offset, comma-separated, in row order.  It needs OUT,
 * OUT.#, OUT.$ and OUT.sa only (the text is restored on the GPU), takes no file argument and holds the suffix array (8 n
 * bytes) on the host while it writes.  --min-records Q, --max-records Q and --unique filter by the distinct records an
 * interval occurs in (debwt_fm_repeats_records, Definition 12; --unique: no record holds the string twice): any of them
 * keeps the record array too, builds the record prefix and adds the column rec behind occ.
 *
 * mums lists the multi-MUMs of the collection: the maximal repeats of at least L bases (--min-len, default 20) that occur
 * exactly once in each of at least Q records (--min-records, default every record) and nowhere else.  stdout: one line
 * "# mums=N min_records=Q longest=LEN", then per multi-MUM len and its occurrences as record:offset, comma-separated,
 * ascending by record; --seq appends the string.  Files and memory as for repeats.
 *
 * count --records adds a column behind the count: the distinct records the pattern occurs in (debwt_fm_record_counts over
 * an uncapped build with the record array; exact patterns on one strand only).
 *
 * graph writes the string graph of the indexed records as GFA 1 (debwt_fm_string_graph): a record that equals an earlier one
 * is a duplicate, one that lies inside a longer record is contained, the others are kept.  One "S J * LN:i:len" line per
 * kept record J (the 0-based number, as extract names records), then one "L a + b + <L>M" line per edge: the longest
 * overlap of at least L bases (default 20) of record a's end with record b's start, strand + only, without the edges that
 * two others explain (a -> j and j -> b laid end to end); --all-edges writes those too.  --states FILE gets
 * J<TAB>kept|duplicate|contained per record.  unitigs follows the unbranched paths of that graph (debwt_fm_unitigs) and
 * writes their sequences as FASTA, ">unitig_N reads=T len=BASES circular=0|1 first=J", in unitig order; a circular unitig is
 * cut where it closes.  Both need OUT, OUT.#, OUT.$ and OUT.sa only (the text is restored on the GPU), take no file
 * argument and write one summary line to stderr.  With --both-strands every read takes part as it is (+) and
 * reverse-complemented (-), from the same index (debwt_fm_string_graph_both, debwt_fm_unitigs_both): S lines and --states
 * stay per read, the links are "L a +|- b +|- <L>M", and of an edge u -> v and its mirror v' -> u' (the same overlap seen
 * from the other strand) the one whose pair of oriented numbers (2 * read + strand) is lower is written; unitigs writes
 * every read once, in one orientation, and first=J+ or first=J- names the first read and its strand.
 * --clean clips the tips and pops the bubbles of the irreducible graph before it is written or walked
 * (debwt_fm_graph_clean): a dead-end chain of at most N reads (--max-tip, default 4) beside a way that goes on, and all but
 * the longest of the unbranched chains of at most N reads (--max-bubble, default 16) that lead from one read to one other,
 * in at most R rounds (--clean-rounds, default 8); any of the three options implies --clean, and --all-edges does not go
 * with it.  The reads removed get no S line and no L line, --states names them clipped or popped, and stderr gets a
 * second summary line.  Without --clean the output is what it was.
 *
 * OUT.sa: 16 little-endian u64 header words -- magic, n, nrec, S, '$' row, the row census of OUT (4 words), the sample
 * count, 6 zero words -- then the samples.  OUT does not carry n (its last word is padded): the header does, and a header
 * that does not match OUT, OUT.# and OUT.$ is refused.
 */
#include <stddef.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <sys/stat.h>

#include "../include/debwt_hip.h"

#define SA_MAGIC 0x3141534657424544ull   /* "DEBWFSA1" */
#define SA_HEADER_WORDS 16

/* the subcommands; bit c of an option's mask (struct option, below) stands for command c */
enum cmd { CMD_INDEX, CMD_COUNT, CMD_LOCATE, CMD_MEMS, CMD_MAP, CMD_PILEUP, CMD_CONSENSUS, CMD_OVERLAPS, CMD_EXTRACT, CMD_KMERS,
           CMD_CORRECT, CMD_SPECTRUM, CMD_LCP, CMD_REPEATS, CMD_MUMS, CMD_DBG, CMD_GRAPH, CMD_UNITIGS, CMD_BIDBG };

/* everything the command line says: set_defaults() fills it, the option table writes into it, the commands read it */
struct query_args {
    enum cmd cmd; const char *name;                                         /* the subcommand */
    const char *out, *file;                                                 /* -i, and the argument that is no option */
    int device;
    uint64_t threads, seed, sa_sample; int iupac;                           /* index, and --ref of the commands that map */
    uint64_t max_hits; uint32_t mismatches, mem_len, flags;                 /* count, locate, mems, overlaps, kmers */
    int search, count_records;                                              /* search: an option of debwt_fm_search was given */
    uint32_t min_overlap, ovl_k, ovl_permille; int no_self, ovl_mm, permille_given;       /* overlaps; min_overlap: graph too */
    const char *ref, *mate; int chain, gap_given, insert_given, no_rescue;  /* map, pileup, consensus */
    debwt_fm_map_opts mo; debwt_fm_chain_opts co; debwt_fm_pair_opts po;
    const char *region, *variants; uint64_t window, min_mapq; debwt_fm_pile_opts call;    /* pileup, consensus */
    int all;                                                                /* extract */
    debwt_fm_correct_opts ko; int k_given, auto_count; const char *report;  /* kmers, correct, spectrum, dbg: ko.k, ko.flags */
    uint32_t bins, at_least, at_most; const char *list; int filter_given;   /* spectrum */
    uint32_t max_lcp, profile_k; const char *lcp_file, *sa_file, *da_file;  /* lcp; max_lcp: repeats too */
    /* repeats, mums.  by_record: --min-records, --max-records or --unique was given (a column `rec` then follows `occ`);
     * min_records 0 stands for 1, and under mums for every record of the index */
    uint32_t min_len, kind; uint64_t min_occ, max_occ, min_records, max_records; int seq, occurrences, unique, by_record, kind_given;
    int fasta;                                                              /* dbg, bidbg */
    int all_edges, both, clean; const char *states; debwt_fm_clean_opts cl; /* graph, unitigs */
};

static void usage(void) {
    fprintf(stderr,
            "usage: deBWT-query index  -i OUT [-t T] [--iupac SEED] [--device D] [--sa S] INPUT.fa[.gz]\n"
            "       deBWT-query count  -i OUT [--device D] [--mismatches K] [--both-strands] [--best] [--records] PATTERNS.fa|.fq\n"
            "       deBWT-query locate -i OUT [--device D] [--max-hits M] [--mismatches K] [--both-strands] [--best] PATTERNS.fa|.fq\n"
            "       deBWT-query mems   -i OUT [--device D] [--min-len L] [--both-strands] [--max-hits M] READS.fa|.fq\n"
            "       deBWT-query overlaps -i OUT [--device D] [--min-overlap L] [--both-strands] [--longest] [--no-self]\n"
            "                          [--max-mismatches K [--max-error-permille R]] READS.fa|.fq\n"
            "       deBWT-query map    -i OUT [--ref INPUT.fa[.gz] [-t T] [--iupac SEED]] [--device D] [--min-len L] [--band W]\n"
            "                          [--max-occ N] [--min-score S] [--chain [--max-gap G]]\n"
            "                          [--mate READS2.fa|.fq [--insert LO,HI] [--no-rescue]] READS.fa|.fq\n"
            "       deBWT-query pileup -i OUT [the options of map] [--min-mapq Q] [--region J[:BEG-END]] [--window N] READS.fa|.fq\n"
            "       deBWT-query consensus -i OUT [the options of map] [--min-mapq Q] [--region J[:BEG-END]] [--window N]\n"
            "                          [--min-depth D] [--min-permille P] [--variants FILE] READS.fa|.fq\n"
            "       deBWT-query extract -i OUT [--device D] --all | REGIONS.txt\n"
            "       deBWT-query kmers  -i OUT -k K [--device D] [--both-strands] READS.fa|.fq\n"
            "       deBWT-query correct -i OUT -k K [--device D] [--min-count T|auto] [--rounds R] [--forward] [--report FILE] READS.fa|.fq\n"
            "       deBWT-query spectrum -i OUT -k K [--device D] [--forward] [--bins N] [--list FILE [--at-least A] [--at-most B]]\n"
            "       deBWT-query lcp    -i OUT [--device D] [--max-lcp C] [--lcp FILE] [--sa FILE] [--da FILE] [--profile K]\n"
            "       deBWT-query repeats -i OUT [--device D] [--min-len L] [--min-occ A] [--max-occ B] [--supermaximal | --intervals]\n"
            "                          [--max-lcp C] [--seq] [--occurrences] [--min-records Q] [--max-records Q] [--unique]\n"
            "       deBWT-query mums   -i OUT [--device D] [--min-len L] [--min-records Q] [--seq]\n"
            "       deBWT-query dbg    -i OUT -k K [--device D] [--fasta]\n"
            "       deBWT-query bidbg  -i OUT -k K [--device D] [--fasta]\n"
            "       deBWT-query graph  -i OUT [--device D] [--min-overlap L] [--all-edges] [--both-strands] [--states FILE]\n"
            "                          [--clean] [--max-tip N] [--max-bubble N] [--clean-rounds R]\n"
            "       deBWT-query unitigs -i OUT [--device D] [--min-overlap L] [--both-strands] [--states FILE]\n"
            "                          [--clean] [--max-tip N] [--max-bubble N] [--clean-rounds R]\n"
            "index writes OUT.sa (the suffix-array samples) and exits 1 when OUT is not the BWT of INPUT;\n"
            "count / locate print name<TAB>count[<TAB>record:offset,...] per pattern of a FASTA or FASTQ file;\n"
            "with --mismatches K (0..4), --both-strands or --best: name<TAB>total<TAB>c0,..,cK (count) or\n"
            "name<TAB>total<TAB>record:offset:strand:mismatches,... (locate);\n"
            "mems prints name<TAB>strand<TAB>qbeg<TAB>qend<TAB>count<TAB>record:offset,... per maximal exact match of at\n"
            "least L bases (default 19);\n"
            "overlaps prints name<TAB>strand<TAB>record<TAB>length<TAB>flags per record that begins with the last `length`\n"
            "(at least L, default 20) bases of the read; flags C (the whole record), W (the whole read), CW or .; --longest\n"
            "keeps the longest overlap per read, strand and record, --no-self drops read i's whole-length overlap with record i;\n"
            "--max-mismatches K (0..4) admits K mismatching columns in an overlap, --max-error-permille R (0..1000) at most\n"
            "R / 1000 of its columns, and a sixth column gives every overlap's mismatches;\n"
            "map prints one PAF line per mapped read (AS:i: score, NM:i: edits, cg:Z: CIGAR); --ref is the FASTA that OUT\n"
            "is the BWT of, without it the text is restored from the index; --chain chains the seeds of a read across diagonals and aligns along the chain (stretches of\n"
            "at most G bases between two seeds, default 5000); --mate maps paired ends, read i of READS2 being the mate of\n"
            "read i of READS (tags pr:A:P|U, tl:i: template length, rs:i:1 rescued mate), --insert LO,HI bounds the template\n"
            "length instead of estimating it, --no-rescue leaves a mate without a seed unmapped;\n"
            "pileup maps the reads as map does, piles the hits of mapping quality Q or more (default 20) up and prints, per\n"
            "position that a read covers, record<TAB>offset (1-based)<TAB>reference base<TAB>depth<TAB>A<TAB>C<TAB>G<TAB>T<TAB>\n"
            "deleted<TAB>insertions behind<TAB>other; consensus prints, per record (>J) or for the region, the called base in\n"
            "upper case, the reference base in lower case where fewer than D reads (default 4) or less than P / 1000 of\n"
            "them (default 600) agree, nothing for a called deletion, and a voted insertion behind its position; --variants\n"
            "FILE gets record<TAB>offset<TAB>ref<TAB>alt (a base, - or +STRING)<TAB>depth<TAB>count; --region walks one record or a\n"
            "part of it (0-based, end exclusive), --window N positions are piled up at a time (default 2^26);\n"
            "extract writes FASTA from the index alone: --all every record under the header >J (its 0-based number), or\n"
            "the regions of REGIONS.txt, one per line, J or J:BEG-END (0-based, end exclusive), under the region as given;\n"
            "kmers prints name<TAB>c0,c1,.. per read, the occurrences of its K-mers (* for a read shorter than K);\n"
            "correct writes the reads as FASTA with the substitution errors fixed that their K-mer counts single out (weak below\n"
            "T occurrences, default 3; at most R rounds, default 4; both strands unless --forward); --report FILE gets\n"
            "name<TAB>status<TAB>fixes<TAB>weak_before<TAB>weak_after, stderr one summary line; --min-count auto takes T from\n"
            "the valley of the spectrum and exits 1 when there is none;\n"
            "spectrum prints # k, # strands, # distinct, # total, # valley, # peak and # est_size (name<TAB>value), then\n"
            "mult<TAB>distinct per non-empty bin of the histogram of the distinct K-mers (K in 1..32; N bins, 2..4096, default\n"
            "256, the last printed as >=N-1; both strands unless --forward); --list FILE gets KMER<TAB>mult of the K-mers of\n"
            "multiplicity A (--at-least, default 1) to B (--at-most), in K-mer order;\n"
            "lcp builds suffix array, LCP array and record array of the collection: --lcp, --sa and --da FILE get them as raw\n"
            "little-endian u32, u64 and u32 arrays of n entries (LCP values cut at separators and capped at C with --max-lcp C);\n"
            "stdout gets # n=N<TAB>max=M<TAB>max_row=R<TAB>prev=J:OFF<TAB>pos=J:OFF<TAB>mean=X and, with --profile K (1..4096, at\n"
            "most C), k<TAB>distinct for k = 1..K, the distinct strings of k bases inside records;\n"
            "repeats lists the maximal repeats of at least L bases (default 20) with A (default 2) to B occurrences, from the\n"
            "LCP array: # intervals=I<TAB>maximal=M<TAB>supermaximal=S<TAB>reported=R<TAB>longest=LEN, then per repeat\n"
            "len<TAB>occ<TAB>S|M|-<TAB>a,c,g,t,s (occurrences behind A, C, G, T, at a record's start)<TAB>record:offset of the\n"
            "first occurrence; --supermaximal lists the supermaximal repeats, --intervals every interval; --seq appends the\n"
            "string, --occurrences every occurrence; --max-lcp C caps the LCP values (L below C); --min-records Q,\n"
            "--max-records Q and --unique (no record holds the string twice) filter by the distinct records of a repeat and add\n"
            "the column rec behind occ;\n"
            "mums lists the multi-MUMs, the maximal repeats of at least L bases (default 20) that occur once in each of at least\n"
            "Q records (default all) and nowhere else: # mums=N<TAB>min_records=Q<TAB>longest=LEN, then per multi-MUM\n"
            "len<TAB>record:offset,... ascending by record; --seq appends the string;\n"
            "count --records adds the distinct records a pattern occurs in behind its count;\n"
            "dbg writes the compacted de Bruijn graph of the K-mers of the collection (forward strand, K in 1..2^32-2) as GFA 1:\n"
            "S<TAB>u<TAB>string<TAB>LN:i:len<TAB>KC:i:k-mer occurrences[<TAB>CL:Z:circular] per unitig, in the order of their first\n"
            "K-mers, L<TAB>a<TAB>+<TAB>b<TAB>+<TAB><K-1>M per edge; --fasta writes the unitigs alone under >uJ nodes=N kc=C [circular];\n"
            "stderr gets one # line with nodes, unitigs, edges, the longest unitig and N50;\n"
            "bidbg writes the graph over both strands (odd K): a K-mer and its reverse complement are one node, S lines in the\n"
            "order of their lowest K-mer that occurs, L<TAB>a<TAB>+|-<TAB>b<TAB>+|-<TAB><K-1>M per edge (- reads the unitig reverse-\n"
            "complemented; an edge and its mirror are both listed), and the # line counts the refused hairpins too;\n"
            "graph writes GFA 1: S lines for the records that are neither duplicates nor contained, L lines a + b + <L>M for the\n"
            "longest overlaps of at least L bases (default 20) that no two other edges explain (--all-edges: all of them);\n"
            "unitigs writes the unbranched paths of that graph as FASTA; --states FILE gets J<TAB>kept|duplicate|contained;\n"
            "--both-strands takes every read on both strands (L a +|- b +|- <L>M, an edge and its mirror written once;\n"
            "first=J+|- in the FASTA headers); --clean first clips dead-end chains of at most N reads (--max-tip, default 4) and\n"
            "pops all but the longest of parallel chains of at most N reads (--max-bubble, default 16), in at most R rounds\n"
            "(--clean-rounds, default 8; each of the three implies --clean; not with --all-edges): the reads removed get no S\n"
            "and no L line and --states names them clipped or popped\n");
}

static int parse_u64(const char *s, uint64_t *out) {
    char *end;
    if (!s || !*s || *s == '-') return -1;
    unsigned long long v = strtoull(s, &end, 10);
    if (*end) return -1;
    *out = v;
    return 0;
}

static char *with_suffix(const char *path, const char *suffix) {
    size_t a = strlen(path), b = strlen(suffix);
    char *p = malloc(a + b + 1);
    if (!p) return NULL;
    memcpy(p, path, a); memcpy(p + a, suffix, b + 1);
    return p;
}

/* a whole file of u64 words; *nwords = its size / 8.  NULL when it cannot be read or its size is not a multiple of 8. */
static uint64_t *read_words(const char *path, uint64_t *nwords) {
    struct stat sb;
    if (stat(path, &sb) || sb.st_size % 8) return NULL;
    *nwords = (uint64_t)sb.st_size / 8;
    uint64_t *w = malloc(*nwords ? *nwords * 8 : 8);
    FILE *f = fopen(path, "rb");
    if (!w || !f) { free(w); if (f) fclose(f); return NULL; }
    if (*nwords && fread(w, 8, *nwords, f) != *nwords) { free(w); fclose(f); return NULL; }
    fclose(f);
    return w;
}

/* rows per 2-bit code of the first n rows of packed words (row j at bits 2*(31-(j&31)) of word j>>5) */
static void census(const uint64_t *w, uint64_t n, uint64_t c[4]) {
    c[0] = c[1] = c[2] = c[3] = 0;
    for (uint64_t i = 0; i < (n + 31) / 32; i++) {
        uint64_t rows = n - i * 32 < 32 ? n - i * 32 : 32;
        uint64_t valid = rows == 32 ? 0x5555555555555555ull : (0x5555555555555555ull << (2 * (32 - rows)));
        uint64_t lo = w[i] & valid, hi = (w[i] >> 1) & valid;
        uint64_t c3 = (uint64_t)__builtin_popcountll(hi & lo), c2 = (uint64_t)__builtin_popcountll(hi & ~lo),
                 c1 = (uint64_t)__builtin_popcountll(~hi & lo);
        c[1] += c1; c[2] += c2; c[3] += c3; c[0] += rows - c1 - c2 - c3;
    }
}

struct rows { uint64_t *words, nwords, *hash, nhash, dollar; };

static int read_rows(const char *out, struct rows *r) {
    char *ph = with_suffix(out, ".#"), *pd = with_suffix(out, ".$");
    uint64_t nd = 0, *d = NULL;
    memset(r, 0, sizeof *r);
    r->words = read_words(out, &r->nwords);
    if (ph) r->hash = read_words(ph, &r->nhash);
    if (pd) d = read_words(pd, &nd);
    int ok = r->words && r->hash && d && nd == 1;
    if (ok) r->dollar = d[0];
    else fprintf(stderr, "cannot read %s, %s and %s (deBWT's output)\n", out, ph ? ph : "OUT.#", pd ? pd : "OUT.$");
    free(ph); free(pd); free(d);
    return ok ? 0 : -1;
}

/* ---- index ---------------------------------------------------------------------------------------------------------- */

static int cmd_index(const struct query_args *A) {
    debwt_config cfg = {32, A->device, 0, 0};
    debwt_ctx *ctx = NULL;
    int rc = debwt_create(&cfg, &ctx);
    if (rc) { fprintf(stderr, "debwt_create: %s\n", debwt_strerror(rc)); return 1; }
    rc = debwt_load_fasta_opts(ctx, A->file, (int)A->threads, A->iupac ? DEBWT_FASTA_IUPAC_RANDOM : 0u, A->seed);
    if (rc) {
        fprintf(stderr, "%s: %s (sequence must be ACGT only unless --iupac is given, records > 32 bases)\n", A->file,
                debwt_last_error(ctx));
        debwt_destroy(ctx);
        return 1;
    }
    debwt_stats st;
    debwt_get_stats(ctx, &st);
    struct rows r;
    if (read_rows(A->out, &r)) { debwt_destroy(ctx); return 1; }
    debwt_fm *fm = NULL;
    if (r.nwords != (st.n + 31) / 32 || r.nhash != st.nrec - 1) {
        fprintf(stderr, "%s is not the BWT of %s: %llu rows / %llu '#' rows expected\n", A->out, A->file,
                (unsigned long long)st.n, (unsigned long long)(st.nrec - 1));
        rc = DEBWT_EINVAL;
    } else {
        rc = debwt_fm_create(ctx, r.words, r.hash, r.dollar, (uint32_t)A->sa_sample, &fm);
        if (rc) fprintf(stderr, "%s is not the BWT of %s: %s\n", A->out, A->file, debwt_last_error(ctx));
    }
    debwt_destroy(ctx);                                   /* the index keeps what it needs */
    int ret = rc ? 1 : 0;
    if (!rc) {
        debwt_fm_info info;
        debwt_fm_info_get(fm, &info);
        uint64_t *buf = malloc((SA_HEADER_WORDS + info.samples) * 8);
        char *psa = with_suffix(A->out, ".sa");
        FILE *f = psa ? fopen(psa, "wb") : NULL;
        if (buf && f) {
            memset(buf, 0, SA_HEADER_WORDS * 8);
            buf[0] = SA_MAGIC; buf[1] = info.n; buf[2] = info.nrec; buf[3] = info.sa_sample; buf[4] = r.dollar;
            memcpy(buf + 5, info.census, 32);
            buf[9] = info.samples;
            rc = debwt_fm_samples(fm, buf + SA_HEADER_WORDS, info.samples);
            if (rc) fprintf(stderr, "debwt_fm_samples: %s\n", debwt_fm_last_error(fm));
            else if (fwrite(buf, 8, SA_HEADER_WORDS + info.samples, f) != SA_HEADER_WORDS + info.samples) rc = DEBWT_EIO;
        } else rc = DEBWT_EIO;
        if (f && fclose(f)) rc = DEBWT_EIO;
        if (rc == DEBWT_EIO) fprintf(stderr, "cannot write %s\n", psa ? psa : "OUT.sa");
        if (!rc) fprintf(stderr, "%s: n = %llu, %llu records, %llu samples (every %llu rows), rank %.1f ms, samples %.1f ms\n",
                         psa, (unsigned long long)info.n, (unsigned long long)info.nrec, (unsigned long long)info.samples,
                         (unsigned long long)info.sa_sample, info.ms_rank, info.ms_samples);
        ret = rc ? 1 : 0;
        free(buf); free(psa);
        debwt_fm_destroy(fm);
    }
    free(r.words); free(r.hash);
    return ret;
}

/* ---- patterns ------------------------------------------------------------------------------------------------------- */

struct patterns {
    char *seq; uint64_t len, cap;          /* sequences concatenated */
    uint64_t *off; char **name; uint64_t n, ncap;
};

static int push_char(struct patterns *p, char c) {
    if (p->len == p->cap) {
        uint64_t nc = p->cap ? 2 * p->cap : 1 << 16;
        char *s = realloc(p->seq, nc);
        if (!s) return -1;
        p->seq = s; p->cap = nc;
    }
    p->seq[p->len++] = c;
    return 0;
}

static int push_record(struct patterns *p, const char *header) {
    if (p->n + 1 >= p->ncap) {
        uint64_t nc = p->ncap ? 2 * p->ncap : 1024;
        uint64_t *o = realloc(p->off, nc * 8);
        if (!o) return -1;
        p->off = o;
        char **nm = realloc(p->name, nc * sizeof(char *));
        if (!nm) return -1;
        p->name = nm; p->ncap = nc;
    }
    size_t l = strcspn(header, " \t\r\n");
    char *nm = malloc(l + 1);
    if (!nm) return -1;
    memcpy(nm, header, l); nm[l] = 0;
    p->name[p->n] = nm;
    p->off[p->n] = p->len;
    p->n++;
    p->off[p->n] = p->len;
    return 0;
}

/* FASTA (sequence over several lines) or FASTQ (4 lines per record), told apart by the first character */
static int read_patterns(const char *path, struct patterns *p) {
    memset(p, 0, sizeof *p);                                /* callers free it whatever comes back */
    FILE *f = fopen(path, "r");
    if (!f) { fprintf(stderr, "cannot open %s\n", path); return -1; }
    char *line = NULL;
    size_t lcap = 0;
    ssize_t l;
    int fastq = -1, err = 0;
    uint64_t lineno = 0;
    while ((l = getline(&line, &lcap, f)) >= 0) {
        lineno++;
        while (l > 0 && (line[l - 1] == '\n' || line[l - 1] == '\r')) line[--l] = 0;
        if (fastq < 0) {
            if (!l) continue;
            if (line[0] != '>' && line[0] != '@') { fprintf(stderr, "%s: not FASTA or FASTQ\n", path); err = 1; break; }
            fastq = line[0] == '@';
        }
        if (fastq) {
            if (!l && (lineno % 4) == 1) { lineno--; continue; }
            switch ((int)(lineno % 4)) {
                case 1:
                    if (line[0] != '@') { fprintf(stderr, "%s:%llu: '@' expected\n", path, (unsigned long long)lineno); err = 1; }
                    else err = push_record(p, line + 1) != 0;
                    break;
                case 2:
                    for (ssize_t i = 0; i < l && !err; i++) err = push_char(p, line[i]) != 0;
                    p->off[p->n] = p->len;
                    break;
                case 3:
                    if (line[0] != '+') { fprintf(stderr, "%s:%llu: '+' expected\n", path, (unsigned long long)lineno); err = 1; }
                    break;
                default: break;
            }
        } else if (l && line[0] == '>') {
            err = push_record(p, line + 1) != 0;
        } else if (p->n) {
            for (ssize_t i = 0; i < l && !err; i++)
                if (line[i] != ' ' && line[i] != '\t') err = push_char(p, line[i]) != 0;
            p->off[p->n] = p->len;
        } else if (l) { fprintf(stderr, "%s: sequence before the first header\n", path); err = 1; }
        if (err) break;
    }
    free(line);
    fclose(f);
    if (!err && !p->off) {                                  /* no record at all: an empty batch */
        p->off = calloc(1, 8);
        if (!p->off) err = 1;
    }
    return err ? -1 : 0;
}

static void free_patterns(struct patterns *p) {
    for (uint64_t i = 0; i < p->n; i++) free(p->name[i]);
    free(p->name); free(p->off); free(p->seq);
}

/* ---- count / locate -------------------------------------------------------------------------------------------------- */

static int open_index(const char *out, int device, debwt_fm **fm) {
    char *psa = with_suffix(out, ".sa");
    uint64_t nsa = 0, *sa = psa ? read_words(psa, &nsa) : NULL;
    struct rows r;
    int ret = 1;
    if (!sa || nsa < SA_HEADER_WORDS || sa[0] != SA_MAGIC) {
        fprintf(stderr, "cannot read %s (made by deBWT-query index)\n", psa ? psa : "OUT.sa");
        free(psa); free(sa);
        return 1;
    }
    if (read_rows(out, &r)) { free(psa); free(sa); return 1; }
    const uint64_t n = sa[1], nrec = sa[2], s = sa[3], dollar = sa[4], nsamp = sa[9];
    uint64_t c[4];
    if (n < 2 || nrec < 1 || !s || nsamp != (n + s - 1) / s || nsa != SA_HEADER_WORDS + nsamp || r.nwords != (n + 31) / 32 ||
        r.nhash != nrec - 1 || r.dollar != dollar) {
        fprintf(stderr, "%s does not belong to %s, %s.# and %s.$\n", psa, out, out, out);
        goto done;
    }
    census(r.words, n, c);
    if (memcmp(c, sa + 5, 32)) { fprintf(stderr, "%s does not belong to %s: the row census differs\n", psa, out); goto done; }
    int rc = debwt_fm_open(device, r.words, n, r.hash, nrec, dollar, sa + SA_HEADER_WORDS, (uint32_t)s, fm);
    if (rc) { fprintf(stderr, "debwt_fm_open: %s\n", debwt_strerror(rc)); goto done; }
    ret = 0;
done:
    free(psa); free(sa); free(r.words); free(r.hash);
    return ret;
}

static int cmp_u64(const void *a, const void *b) {
    uint64_t x = *(const uint64_t *)a, y = *(const uint64_t *)b;
    return x < y ? -1 : x > y;
}

static int cmd_query(const struct query_args *A) {
    const int locate = A->cmd == CMD_LOCATE;
    struct patterns P;
    if (read_patterns(A->file, &P)) { free_patterns(&P); return 1; }
    debwt_fm *fm = NULL;
    if (open_index(A->out, A->device, &fm)) { free_patterns(&P); return 1; }
    int ret = 1;
    uint64_t *ranges = malloc((P.n ? P.n : 1) * 16), *oo = malloc((P.n + 1) * 8), *pos = NULL, *starts = NULL;
    uint64_t *nrecs = A->count_records ? malloc((P.n ? P.n : 1) * 8) : NULL;
    debwt_fm_info info;
    debwt_fm_info_get(fm, &info);
    starts = malloc(info.nrec * 8);
    if (!ranges || !oo || !starts || (A->count_records && !nrecs)) { fprintf(stderr, "out of memory\n"); goto done; }
    int rc = debwt_fm_count(fm, P.seq, P.off, P.n, ranges);
    if (!rc) rc = debwt_fm_record_starts(fm, starts, info.nrec);
    /* the range of a pattern is closed (Definition 12) on the uncapped array, whatever its length */
    if (!rc && A->count_records) rc = debwt_fm_esa_build(fm, 0, DEBWT_FM_ESA_DA);
    if (!rc && A->count_records) rc = debwt_fm_records_build(fm);
    if (!rc && A->count_records) rc = debwt_fm_record_counts(fm, ranges, P.n, nrecs);
    if (!rc && locate) {
        uint64_t total = 0;
        for (uint64_t i = 0; i < P.n; i++) {
            uint64_t c = ranges[2 * i + 1] - ranges[2 * i];
            total += A->max_hits && c > A->max_hits ? A->max_hits : c;
        }
        pos = malloc((total ? total : 1) * 8);
        if (!pos) { fprintf(stderr, "out of memory\n"); goto done; }
        rc = debwt_fm_locate(fm, ranges, P.n, A->max_hits, oo, pos, total);
    }
    if (rc) { fprintf(stderr, "%s\n", debwt_fm_last_error(fm)); goto done; }
    for (uint64_t i = 0; i < P.n; i++) {
        printf("%s\t%llu", P.name[i], (unsigned long long)(ranges[2 * i + 1] - ranges[2 * i]));
        if (A->count_records) printf("\t%llu", (unsigned long long)nrecs[i]);
        if (locate) {
            uint64_t *a = pos + oo[i], m = oo[i + 1] - oo[i], rec = 0;
            qsort(a, m, 8, cmp_u64);
            putchar('\t');
            for (uint64_t j = 0; j < m; j++) {
                while (rec + 1 < info.nrec && starts[rec + 1] <= a[j]) rec++;
                printf("%s%llu:%llu", j ? "," : "", (unsigned long long)rec, (unsigned long long)(a[j] - starts[rec]));
            }
        }
        putchar('\n');
    }
    ret = fflush(stdout) ? 1 : 0;
done:
    free(ranges); free(oo); free(pos); free(starts); free(nrecs);
    debwt_fm_destroy(fm);
    free_patterns(&P);
    return ret;
}

/* one located occurrence of a search hit */
struct occ { uint64_t rec, off; uint32_t strand, mm; };

static int cmp_occ(const void *a, const void *b) {
    const struct occ *x = a, *y = b;
    if (x->rec != y->rec) return x->rec < y->rec ? -1 : 1;
    if (x->off != y->off) return x->off < y->off ? -1 : 1;
    return (x->strand > y->strand) - (x->strand < y->strand);
}

static int cmd_search(const struct query_args *A) {
    const int locate = A->cmd == CMD_LOCATE;
    struct patterns P;
    if (read_patterns(A->file, &P)) { free_patterns(&P); return 1; }
    debwt_fm *fm = NULL;
    if (open_index(A->out, A->device, &fm)) { free_patterns(&P); return 1; }
    int ret = 1, rc;
    uint64_t cap = 4 * P.n + 16, *hoff = malloc((P.n + 1) * 8), *ranges = NULL, *oo = NULL, *pos = NULL, *starts = NULL;
    uint32_t *info = NULL;
    struct occ *occ = NULL;
    debwt_fm_info fi;
    debwt_fm_info_get(fm, &fi);
    starts = malloc(fi.nrec * 8);
    if (!hoff || !starts) { fprintf(stderr, "out of memory\n"); goto done; }
    for (;;) {                                            /* grow to the exact hit count on DEBWT_ERANGE */
        free(ranges); free(info);
        ranges = malloc(cap * 16); info = malloc(cap * 4);
        if (!ranges || !info) { fprintf(stderr, "out of memory\n"); goto done; }
        rc = debwt_fm_search(fm, P.seq, P.off, P.n, A->mismatches, A->flags, hoff, ranges, info, cap);
        if (rc == DEBWT_ERANGE && hoff[P.n] > cap) { cap = hoff[P.n]; continue; }
        break;
    }
    if (!rc) rc = debwt_fm_record_starts(fm, starts, fi.nrec);
    const uint64_t nh = rc ? 0 : hoff[P.n];
    uint64_t total = 0;
    for (uint64_t h = 0; h < nh; h++) total += ranges[2 * h + 1] - ranges[2 * h];
    if (!rc && locate) {
        oo = malloc((nh + 1) * 8); pos = malloc((total ? total : 1) * 8); occ = malloc((total ? total : 1) * sizeof *occ);
        if (!oo || !pos || !occ) { fprintf(stderr, "out of memory\n"); goto done; }
        rc = debwt_fm_locate(fm, ranges, nh, 0, oo, pos, total);
    }
    if (rc) { fprintf(stderr, "%s\n", debwt_fm_last_error(fm)); goto done; }
    for (uint64_t i = 0; i < P.n; i++) {
        uint64_t per[5] = {0, 0, 0, 0, 0}, t = 0;
        for (uint64_t h = hoff[i]; h < hoff[i + 1]; h++) {
            const uint64_t c = ranges[2 * h + 1] - ranges[2 * h];
            per[info[h] & 0xFF] += c; t += c;
        }
        printf("%s\t%llu\t", P.name[i], (unsigned long long)t);
        if (!locate) {
            for (uint32_t k = 0; k <= A->mismatches; k++) printf("%s%llu", k ? "," : "", (unsigned long long)per[k]);
        } else {
            uint64_t m = 0;
            for (uint64_t h = hoff[i]; h < hoff[i + 1]; h++)
                for (uint64_t j = oo[h]; j < oo[h + 1]; j++) {
                    uint64_t lo = 0, hi = fi.nrec;             /* the record: last start <= position */
                    while (hi - lo > 1) { uint64_t mid = (lo + hi) / 2; if (starts[mid] <= pos[j]) lo = mid; else hi = mid; }
                    occ[m].rec = lo; occ[m].off = pos[j] - starts[lo]; occ[m].strand = (info[h] >> 8) & 1; occ[m].mm = info[h] & 0xFF;
                    m++;
                }
            qsort(occ, m, sizeof *occ, cmp_occ);
            if (A->max_hits && m > A->max_hits) m = A->max_hits;
            for (uint64_t j = 0; j < m; j++)
                printf("%s%llu:%llu:%c:%u", j ? "," : "", (unsigned long long)occ[j].rec, (unsigned long long)occ[j].off,
                       occ[j].strand ? '-' : '+', occ[j].mm);
        }
        putchar('\n');
    }
    ret = fflush(stdout) ? 1 : 0;
done:
    free(hoff); free(ranges); free(info); free(oo); free(pos); free(occ); free(starts);
    debwt_fm_destroy(fm);
    free_patterns(&P);
    return ret;
}

static int cmd_mems(const struct query_args *A) {
    struct patterns P;
    if (read_patterns(A->file, &P)) { free_patterns(&P); return 1; }
    debwt_fm *fm = NULL;
    if (open_index(A->out, A->device, &fm)) { free_patterns(&P); return 1; }
    int ret = 1, rc;
    uint64_t cap = 4 * P.n + 16, *moff = malloc((P.n + 1) * 8), *ranges = NULL, *oo = NULL, *pos = NULL, *starts = NULL;
    uint32_t *spans = NULL;
    uint8_t *strand = NULL;
    debwt_fm_info fi;
    debwt_fm_info_get(fm, &fi);
    starts = malloc(fi.nrec * 8);
    if (!moff || !starts) { fprintf(stderr, "out of memory\n"); goto done; }
    for (;;) {                                            /* grow to the exact MEM count on DEBWT_ERANGE */
        free(spans); free(ranges); free(strand);
        spans = malloc(cap * 8); ranges = malloc(cap * 16); strand = malloc(cap);
        if (!spans || !ranges || !strand) { fprintf(stderr, "out of memory\n"); goto done; }
        rc = debwt_fm_mems(fm, P.seq, P.off, P.n, A->mem_len, A->flags, moff, spans, ranges, strand, cap);
        if (rc == DEBWT_ERANGE && moff[P.n] > cap) { cap = moff[P.n]; continue; }
        break;
    }
    if (!rc) rc = debwt_fm_record_starts(fm, starts, fi.nrec);
    const uint64_t nm = rc ? 0 : moff[P.n];
    uint64_t total = 0;
    for (uint64_t h = 0; h < nm; h++) {
        const uint64_t c = ranges[2 * h + 1] - ranges[2 * h];
        total += A->max_hits && c > A->max_hits ? A->max_hits : c;
    }
    if (!rc) {
        oo = malloc((nm + 1) * 8); pos = malloc((total ? total : 1) * 8);
        if (!oo || !pos) { fprintf(stderr, "out of memory\n"); goto done; }
        rc = debwt_fm_locate(fm, ranges, nm, A->max_hits, oo, pos, total);
    }
    if (rc) { fprintf(stderr, "%s\n", debwt_fm_last_error(fm)); goto done; }
    for (uint64_t i = 0; i < P.n; i++)
        for (uint64_t h = moff[i]; h < moff[i + 1]; h++) {
            uint64_t *a = pos + oo[h], m = oo[h + 1] - oo[h], rec = 0;
            qsort(a, m, 8, cmp_u64);
            printf("%s\t%c\t%u\t%u\t%llu\t", P.name[i], strand[h] ? '-' : '+', spans[2 * h], spans[2 * h + 1],
                   (unsigned long long)(ranges[2 * h + 1] - ranges[2 * h]));
            for (uint64_t j = 0; j < m; j++) {
                while (rec + 1 < fi.nrec && starts[rec + 1] <= a[j]) rec++;
                printf("%s%llu:%llu", j ? "," : "", (unsigned long long)rec, (unsigned long long)(a[j] - starts[rec]));
            }
            putchar('\n');
        }
    ret = fflush(stdout) ? 1 : 0;
done:
    free(moff); free(spans); free(ranges); free(strand); free(oo); free(pos); free(starts);
    debwt_fm_destroy(fm);
    free_patterns(&P);
    return ret;
}

/* mm: --max-mismatches was given (the call with a mismatch budget and the sixth column) */
static int cmd_overlaps(const struct query_args *A) {
    struct patterns P;
    if (read_patterns(A->file, &P)) { free_patterns(&P); return 1; }
    debwt_fm *fm = NULL;
    if (open_index(A->out, A->device, &fm)) { free_patterns(&P); return 1; }
    int ret = 1, rc;
    uint64_t cap = 4 * P.n + 16, *hoff = malloc((P.n + 1) * 8);
    debwt_fm_overlap *hits = NULL;
    if (!hoff) { fprintf(stderr, "out of memory\n"); goto done; }
    for (;;) {                                            /* grow to the exact hit count on DEBWT_ERANGE */
        free(hits);
        hits = malloc(cap * sizeof *hits);
        if (!hits) { fprintf(stderr, "out of memory\n"); goto done; }
        rc = A->ovl_mm ? debwt_fm_overlaps_mm(fm, P.seq, P.off, P.n, A->min_overlap, A->ovl_k, A->ovl_permille, A->flags, hoff, hits, cap)
                : debwt_fm_overlaps(fm, P.seq, P.off, P.n, A->min_overlap, A->flags, hoff, hits, cap);
        if (rc == DEBWT_ERANGE && hoff[P.n] > cap) { cap = hoff[P.n]; continue; }
        break;
    }
    if (rc) { fprintf(stderr, "%s\n", debwt_fm_last_error(fm)); goto done; }
    for (uint64_t i = 0; i < P.n; i++) {
        const uint64_t m = P.off[i + 1] - P.off[i];
        for (uint64_t h = hoff[i]; h < hoff[i + 1]; h++) {
            const debwt_fm_overlap *o = hits + h;
            if (A->no_self && !o->strand && o->record == i && o->length == m) continue;
            printf("%s\t%c\t%u\t%u\t%s", P.name[i], o->strand ? '-' : '+', o->record, o->length,
                   (o->flags & 3u) == 3u ? "CW" : (o->flags & DEBWT_FM_OVERLAP_CONTAINS) ? "C" :
                   (o->flags & DEBWT_FM_OVERLAP_WHOLE) ? "W" : ".");
            if (A->ovl_mm) printf("\t%u", DEBWT_FM_OVERLAP_MM(o->flags));
            putchar('\n');
        }
    }
    ret = fflush(stdout) ? 1 : 0;
done:
    free(hoff); free(hits);
    debwt_fm_destroy(fm);
    free_patterns(&P);
    return ret;
}

/* ---- map ------------------------------------------------------------------------------------------------------------- */

/* the PAF columns and the tags AS, NM, cg of a mapped read, without the line's end */
static void paf_line(const char *name, uint64_t m, const debwt_fm_hit *h, const uint64_t *starts, const uint32_t *cig,
                     uint64_t c0, uint64_t c1) {
    const int rev = (h->flags & DEBWT_FM_MAP_REVERSE) != 0;
    uint64_t cols = 0, gaps = 0, mcols = 0;
    for (uint64_t k = c0; k < c1; k++) {
        cols += cig[k] >> 4;
        if (cig[k] & 15) gaps += cig[k] >> 4; else mcols += cig[k] >> 4;
    }
    printf("%s\t%llu\t%llu\t%llu\t%c\t%u\t%llu\t%llu\t%llu\t%llu\t%llu\t%u\tAS:i:%d\tNM:i:%u\tcg:Z:", name,
           (unsigned long long)m, (unsigned long long)(rev ? m - h->qend : h->qbeg),
           (unsigned long long)(rev ? m - h->qbeg : h->qend), rev ? '-' : '+', h->record,
           (unsigned long long)(starts[h->record + 1] - 1 - starts[h->record]), (unsigned long long)h->offset,
           (unsigned long long)(h->offset + (h->tend - h->tbeg)), (unsigned long long)(mcols - (h->edits - gaps)),
           (unsigned long long)cols, h->mapq, h->score, h->edits);
    for (uint64_t k = c0; k < c1; k++) printf("%u%c", cig[k] >> 4, "MID"[cig[k] & 3]);
}

/* the text the mappers read: --ref packed as index packs it and checked against the index, or, without --ref, restored
 * from the index itself */
static int map_text(debwt_fm *fm, const struct query_args *A, const debwt_fm_info *fi, debwt_packed_text *pt) {
    const char *out = A->out, *ref = A->ref;
    char err[256] = "";
    int rc;
    if (!ref) {
        rc = debwt_fm_restore_text(fm);
        if (rc) fprintf(stderr, "%s.sa does not restore the text of %s: %s\n", out, out, debwt_fm_last_error(fm));
        return rc ? -1 : 0;
    }
    rc = debwt_pack_fasta_opts(ref, (int)A->threads, A->iupac ? DEBWT_FASTA_IUPAC_RANDOM : 0u, A->seed, pt, err, sizeof err);
    if (rc) {
        fprintf(stderr, "%s: %s (sequence must be ACGT only unless --iupac is given, records > 32 bases)\n", ref, err);
        return -1;
    }
    if (pt->n != fi->n || pt->nrec != fi->nrec) {
        fprintf(stderr, "%s is not the text of %s: %llu symbols in %llu records, the index has %llu in %llu\n", ref, out,
                (unsigned long long)pt->n, (unsigned long long)pt->nrec, (unsigned long long)fi->n, (unsigned long long)fi->nrec);
        return -1;
    }
    rc = debwt_fm_attach_text(fm, NULL, pt->words, pt->sep);
    if (rc) { fprintf(stderr, "%s is not the text of %s: %s\n", ref, out, debwt_fm_last_error(fm)); return -1; }
    return 0;
}

static int cmd_map(const struct query_args *A) {
    struct patterns P;
    if (read_patterns(A->file, &P)) { free_patterns(&P); return 1; }
    debwt_fm *fm = NULL;
    if (open_index(A->out, A->device, &fm)) { free_patterns(&P); return 1; }
    int ret = 1, rc;
    debwt_packed_text pt;
    memset(&pt, 0, sizeof pt);
    uint64_t cap = 4 * P.n + 16, *coff = malloc((P.n + 1) * 8), *starts = NULL;
    uint32_t *cig = NULL;
    debwt_fm_hit *hits = malloc((P.n ? P.n : 1) * sizeof *hits);
    debwt_fm_info fi;
    debwt_fm_info_get(fm, &fi);
    starts = malloc((fi.nrec + 1) * 8);
    if (!coff || !hits || !starts) { fprintf(stderr, "out of memory\n"); goto done; }
    if (map_text(fm, A, &fi, &pt)) goto done;
    for (;;) {                                            /* grow to the exact op count on DEBWT_ERANGE */
        free(cig);
        cig = malloc(cap * 4);
        if (!cig) { fprintf(stderr, "out of memory\n"); goto done; }
        if (A->chain) {
            debwt_fm_chain_opts co;
            debwt_fm_chain_defaults(&co);
            co.map = A->mo;
            co.max_gap = A->co.max_gap;
            rc = debwt_fm_map_chained(fm, P.seq, P.off, P.n, &co, hits, coff, cig, cap, NULL, NULL, 0);
        } else {
            rc = debwt_fm_map(fm, P.seq, P.off, P.n, &A->mo, hits, coff, cig, cap);
        }
        if (rc == DEBWT_ERANGE && coff[P.n] > cap) { cap = coff[P.n]; continue; }
        break;
    }
    if (!rc) rc = debwt_fm_record_starts(fm, starts, fi.nrec);
    if (rc) { fprintf(stderr, "%s\n", debwt_fm_last_error(fm)); goto done; }
    starts[fi.nrec] = fi.n;                               /* record r holds starts[r + 1] - 1 - starts[r] bases */
    for (uint64_t i = 0; i < P.n; i++) {
        if (hits[i].flags & DEBWT_FM_MAP_UNMAPPED) continue;
        paf_line(P.name[i], P.off[i + 1] - P.off[i], &hits[i], starts, cig, coff[i], coff[i + 1]);
        putchar('\n');
    }
    ret = fflush(stdout) ? 1 : 0;
done:
    debwt_free_packed(&pt);
    free(coff); free(cig); free(hits); free(starts);
    debwt_fm_destroy(fm);
    free_patterns(&P);
    return ret;
}

/* ---- map --mate: paired ends ----------------------------------------------------------------------------------------- */

/* the pair options of the command line: they carry the map options, and --no-rescue rescues no mate */
static debwt_fm_pair_opts pair_opts(const struct query_args *A) {
    debwt_fm_pair_opts po = A->po;
    po.map = A->mo;
    if (A->no_rescue) po.max_rescue = 0;
    return po;
}

static int cmd_map_pairs(const struct query_args *A) {
    const debwt_fm_pair_opts po = pair_opts(A);
    struct patterns P, M, B;                              /* mates 1, mates 2, both interleaved (names stay in P and M) */
    memset(&P, 0, sizeof P); memset(&M, 0, sizeof M); memset(&B, 0, sizeof B);
    if (read_patterns(A->file, &P)) return 1;
    if (read_patterns(A->mate, &M)) { free_patterns(&P); return 1; }
    if (P.n != M.n) {
        fprintf(stderr, "--mate: %s holds %llu reads, %s holds %llu: read i of one is the mate of read i of the other\n", A->mate,
                (unsigned long long)M.n, A->file, (unsigned long long)P.n);
        free_patterns(&P); free_patterns(&M);
        return 1;
    }
    const uint64_t np = P.n, nr = 2 * np;
    debwt_fm *fm = NULL;
    if (open_index(A->out, A->device, &fm)) { free_patterns(&P); free_patterns(&M); return 1; }
    int ret = 1, rc;
    debwt_packed_text pt;
    memset(&pt, 0, sizeof pt);
    uint64_t cap = 4 * nr + 16, *coff = malloc((nr + 1) * 8), *starts = NULL;
    uint32_t *cig = NULL;
    debwt_fm_hit *hits = malloc((nr ? nr : 1) * sizeof *hits);
    debwt_fm_pair_info *info = malloc((np ? np : 1) * sizeof *info);
    debwt_fm_info fi;
    debwt_fm_info_get(fm, &fi);
    starts = malloc((fi.nrec + 1) * 8);
    B.seq = malloc(P.len + M.len + 1);
    B.off = malloc((nr + 1) * 8);
    if (!coff || !hits || !info || !starts || !B.seq || !B.off) { fprintf(stderr, "out of memory\n"); goto done; }
    B.off[0] = 0;
    for (uint64_t i = 0; i < np; i++) {
        const uint64_t l1 = P.off[i + 1] - P.off[i], l2 = M.off[i + 1] - M.off[i];
        memcpy(B.seq + B.off[2 * i], P.seq + P.off[i], l1);
        B.off[2 * i + 1] = B.off[2 * i] + l1;
        memcpy(B.seq + B.off[2 * i + 1], M.seq + M.off[i], l2);
        B.off[2 * i + 2] = B.off[2 * i + 1] + l2;
    }
    if (map_text(fm, A, &fi, &pt)) goto done;
    for (;;) {                                            /* grow to the exact op count on DEBWT_ERANGE */
        free(cig);
        cig = malloc(cap * 4);
        if (!cig) { fprintf(stderr, "out of memory\n"); goto done; }
        rc = debwt_fm_map_pairs(fm, B.seq, B.off, np, &po, hits, info, coff, cig, cap);
        if (rc == DEBWT_ERANGE && coff[nr] > cap) { cap = coff[nr]; continue; }
        break;
    }
    if (!rc) rc = debwt_fm_record_starts(fm, starts, fi.nrec);
    if (rc) { fprintf(stderr, "%s\n", debwt_fm_last_error(fm)); goto done; }
    starts[fi.nrec] = fi.n;
    for (uint64_t i = 0; i < nr; i++) {
        const debwt_fm_hit *h = &hits[i];
        if (h->flags & DEBWT_FM_MAP_UNMAPPED) continue;
        paf_line(i & 1 ? M.name[i / 2] : P.name[i / 2], B.off[i + 1] - B.off[i], h, starts, cig, coff[i], coff[i + 1]);
        printf("\tpr:A:%c", h->flags & DEBWT_FM_MAP_PROPER ? 'P' : 'U');
        if (h->flags & DEBWT_FM_MAP_PROPER)
            printf("\ttl:i:%lld", (long long)(h->flags & DEBWT_FM_MAP_REVERSE ? -info[i / 2].tlen : info[i / 2].tlen));
        if (h->flags & DEBWT_FM_MAP_RESCUED) printf("\trs:i:1");
        putchar('\n');
    }
    ret = fflush(stdout) ? 1 : 0;
done:
    debwt_free_packed(&pt);
    free(coff); free(cig); free(hits); free(info); free(starts);
    debwt_fm_destroy(fm);
    free(B.seq); free(B.off);
    free_patterns(&P); free_patterns(&M);
    return ret;
}

/* ---- extract ---------------------------------------------------------------------------------------------------------- */

#define EXTRACT_BATCH_BYTES (64ull << 20)
#define EXTRACT_BATCH_JOBS (1ull << 16)

struct regions { debwt_fm_extract_job *job; char **name; uint64_t n, cap; };

static int push_region(struct regions *R, const char *name, uint64_t rec, uint64_t beg, uint64_t len) {
    if (R->n == R->cap) {
        uint64_t nc = R->cap ? 2 * R->cap : 1024;
        debwt_fm_extract_job *j = realloc(R->job, nc * sizeof *j);
        if (!j) return -1;
        R->job = j;
        char **nm = realloc(R->name, nc * sizeof *nm);
        if (!nm) return -1;
        R->name = nm; R->cap = nc;
    }
    R->name[R->n] = NULL;
    if (name && !(R->name[R->n] = strdup(name))) return -1;
    R->job[R->n].record = (uint32_t)rec; R->job[R->n].reserved = 0; R->job[R->n].offset = beg; R->job[R->n].length = len;
    R->n++;
    return 0;
}

/* J or J:BEG-END into (rec, beg, end); whole: no interval was given */
static int parse_region(const char *s, uint64_t *rec, uint64_t *beg, uint64_t *end, int *whole) {
    char buf[64];
    const char *colon = strchr(s, ':');
    *whole = !colon;
    if (!colon) return parse_u64(s, rec);
    const char *dash = strchr(colon + 1, '-');
    if (!dash || (size_t)(colon - s) >= sizeof buf || (size_t)(dash - colon - 1) >= sizeof buf) return -1;
    memcpy(buf, s, (size_t)(colon - s)); buf[colon - s] = 0;
    if (parse_u64(buf, rec)) return -1;
    memcpy(buf, colon + 1, (size_t)(dash - colon - 1)); buf[dash - colon - 1] = 0;
    if (parse_u64(buf, beg) || parse_u64(dash + 1, end)) return -1;
    return 0;
}

static int cmd_extract(const struct query_args *A) {
    debwt_fm *fm = NULL;
    struct regions R;
    memset(&R, 0, sizeof R);
    int ret = 1, rc = 0;
    uint64_t *starts = NULL, *off = NULL;
    char *bases = NULL, *line = NULL;
    FILE *f = NULL;
    if (A->file && !(f = fopen(A->file, "r"))) { fprintf(stderr, "cannot open %s\n", A->file); return 1; }
    if (open_index(A->out, A->device, &fm)) { if (f) fclose(f); return 1; }
    debwt_fm_info fi;
    debwt_fm_info_get(fm, &fi);
    starts = malloc((fi.nrec + 1) * 8);
    if (!starts) { fprintf(stderr, "out of memory\n"); goto done; }
    rc = debwt_fm_record_starts(fm, starts, fi.nrec);
    if (rc) { fprintf(stderr, "%s\n", debwt_fm_last_error(fm)); goto done; }
    starts[fi.nrec] = fi.n;                               /* record r holds starts[r + 1] - 1 - starts[r] bases */
    if (fi.nrec >> 32) { fprintf(stderr, "extract: 2^32 records or more\n"); goto done; }
    if (f) {
        size_t lcap = 0;
        ssize_t l;
        uint64_t lineno = 0;
        while ((l = getline(&line, &lcap, f)) >= 0) {
            lineno++;
            while (l > 0 && (line[l - 1] == '\n' || line[l - 1] == '\r' || line[l - 1] == ' ' || line[l - 1] == '\t')) line[--l] = 0;
            if (!l) continue;
            uint64_t rec = 0, beg = 0, end = 0;
            int whole = 0;
            if (parse_region(line, &rec, &beg, &end, &whole)) {
                fprintf(stderr, "%s:%llu: '%s' is not a region (J or J:BEG-END)\n", A->file, (unsigned long long)lineno, line);
                goto done;
            }
            const uint64_t len = rec < fi.nrec ? starts[rec + 1] - 1 - starts[rec] : 0;
            if (whole) end = len;
            if (rec >= fi.nrec || beg > end || end > len) {
                fprintf(stderr, "%s:%llu: region '%s' lies outside its record (%llu records; record %llu holds %llu bases)\n", A->file,
                        (unsigned long long)lineno, line, (unsigned long long)fi.nrec, (unsigned long long)rec, (unsigned long long)len);
                goto done;
            }
            if (push_region(&R, line, rec, beg, end - beg)) { fprintf(stderr, "out of memory\n"); goto done; }
        }
    }
    /* --all: the records are the jobs, made batch by batch; REGIONS: the jobs read above */
    const uint64_t njobs = f ? R.n : fi.nrec;
    off = malloc((EXTRACT_BATCH_JOBS + 1) * 8);
    debwt_fm_extract_job *jb = f ? NULL : malloc(EXTRACT_BATCH_JOBS * sizeof *jb);
    uint64_t bcap = 0;
    if (!off || (!f && !jb)) { fprintf(stderr, "out of memory\n"); free(jb); goto done; }
    for (uint64_t j0 = 0; j0 < njobs && !rc;) {
        uint64_t j1 = j0, bytes = 0;
        while (j1 < njobs && j1 - j0 < EXTRACT_BATCH_JOBS) {  /* at least one job, however long */
            const uint64_t l = f ? R.job[j1].length : starts[j1 + 1] - 1 - starts[j1];
            if (j1 > j0 && bytes + l > EXTRACT_BATCH_BYTES) break;
            if (!f) { jb[j1 - j0].record = (uint32_t)j1; jb[j1 - j0].reserved = 0; jb[j1 - j0].offset = 0; jb[j1 - j0].length = l; }
            bytes += l; j1++;
        }
        if (bytes > bcap) {
            free(bases);
            bases = malloc(bytes);
            bcap = bases ? bytes : 0;
            if (!bases) { fprintf(stderr, "out of memory\n"); rc = DEBWT_ENOMEM; break; }
        }
        rc = debwt_fm_extract(fm, f ? R.job + j0 : jb, j1 - j0, off, bases, bcap);
        if (rc) { fprintf(stderr, "%s\n", debwt_fm_last_error(fm)); break; }
        for (uint64_t j = j0; j < j1; j++) {
            if (f) printf(">%s\n", R.name[j]); else printf(">%llu\n", (unsigned long long)j);
            fwrite(bases + off[j - j0], 1, off[j - j0 + 1] - off[j - j0], stdout);
            putchar('\n');
        }
        j0 = j1;
    }
    free(jb);
    if (!rc) ret = fflush(stdout) ? 1 : 0;
done:
    if (f) fclose(f);
    for (uint64_t i = 0; i < R.n; i++) free(R.name[i]);
    free(R.name); free(R.job); free(starts); free(off); free(bases); free(line);
    debwt_fm_destroy(fm);
    return ret;
}

/* ---- pileup / consensus ----------------------------------------------------------------------------------------------- */

#define PILE_BATCH_ALNS (1ull << 20)

/* reads -> alignments once (map, map --chain or map --mate), kept on the host; then the text is walked in windows of
 * --window positions: the alignments are piled up in batches with DEBWT_FM_PILE_ADD, the table is fetched (pileup) or
 * called and turned into consensus and variants (consensus) */
static int cmd_pile(const struct query_args *A) {
    const int consensus = A->cmd == CMD_CONSENSUS;
    const debwt_fm_pair_opts po = pair_opts(A);
    struct patterns P, M, B;
    memset(&P, 0, sizeof P); memset(&M, 0, sizeof M); memset(&B, 0, sizeof B);
    if (read_patterns(A->file, &P)) { free_patterns(&P); return 1; }
    if (A->mate && read_patterns(A->mate, &M)) { free_patterns(&P); free_patterns(&M); return 1; }
    if (A->mate && P.n != M.n) {
        fprintf(stderr, "--mate: %s holds %llu reads, %s holds %llu\n", A->mate, (unsigned long long)M.n, A->file, (unsigned long long)P.n);
        free_patterns(&P); free_patterns(&M);
        return 1;
    }
    debwt_fm *fm = NULL;
    if (open_index(A->out, A->device, &fm)) { free_patterns(&P); free_patterns(&M); return 1; }
    int ret = 1, rc = 0;
    debwt_packed_text pt;
    memset(&pt, 0, sizeof pt);
    const uint64_t nr = A->mate ? 2 * P.n : P.n;
    const char *seq = P.seq;
    const uint64_t *off = P.off;
    uint64_t cap = 4 * nr + 16, *coff = malloc((nr + 1) * 8), *starts = NULL, *acoff = NULL, *ooff = NULL, *vt = NULL, *ioff = NULL;
    uint32_t *cig = NULL, *acig = NULL, *counts = NULL, *isup = NULL, *idep = NULL;
    uint8_t *calls = NULL, *refb = NULL;
    char *cons = NULL, *ibases = NULL;
    debwt_fm_hit *hits = malloc((nr ? nr : 1) * sizeof *hits);
    debwt_fm_pair_info *info = A->mate ? malloc((P.n ? P.n : 1) * sizeof *info) : NULL;
    debwt_fm_pile_aln *alns = NULL, *bal = NULL;
    debwt_fm_variant *vars = NULL;
    debwt_fm_ins_event *ev = NULL;
    FILE *vf = NULL;
    debwt_fm_info fi;
    debwt_fm_info_get(fm, &fi);
    starts = malloc((fi.nrec + 1) * 8);
    ooff = malloc((fi.nrec + 1) * 8);
    if (!coff || !hits || !starts || !ooff || (A->mate && !info)) { fprintf(stderr, "out of memory\n"); goto done; }
    if (A->mate) {                                        /* both mates interleaved, as map --mate does */
        B.seq = malloc(P.len + M.len + 1);
        B.off = malloc((nr + 1) * 8);
        if (!B.seq || !B.off) { fprintf(stderr, "out of memory\n"); goto done; }
        B.off[0] = 0;
        for (uint64_t i = 0; i < P.n; i++) {
            const uint64_t l1 = P.off[i + 1] - P.off[i], l2 = M.off[i + 1] - M.off[i];
            memcpy(B.seq + B.off[2 * i], P.seq + P.off[i], l1);
            B.off[2 * i + 1] = B.off[2 * i] + l1;
            memcpy(B.seq + B.off[2 * i + 1], M.seq + M.off[i], l2);
            B.off[2 * i + 2] = B.off[2 * i + 1] + l2;
        }
        seq = B.seq; off = B.off;
    }
    if (map_text(fm, A, &fi, &pt)) goto done;
    for (;;) {                                            /* grow to the exact op count on DEBWT_ERANGE */
        free(cig);
        cig = malloc(cap * 4);
        if (!cig) { fprintf(stderr, "out of memory\n"); goto done; }
        if (A->mate) rc = debwt_fm_map_pairs(fm, seq, off, P.n, &po, hits, info, coff, cig, cap);
        else if (A->chain) {
            debwt_fm_chain_opts co;
            debwt_fm_chain_defaults(&co);
            co.map = A->mo;
            co.max_gap = A->co.max_gap;
            rc = debwt_fm_map_chained(fm, seq, off, nr, &co, hits, coff, cig, cap, NULL, NULL, 0);
        } else rc = debwt_fm_map(fm, seq, off, nr, &A->mo, hits, coff, cig, cap);
        if (rc == DEBWT_ERANGE && coff[nr] > cap) { cap = coff[nr]; continue; }
        break;
    }
    if (!rc) rc = debwt_fm_record_starts(fm, starts, fi.nrec);
    if (rc) { fprintf(stderr, "%s\n", debwt_fm_last_error(fm)); goto done; }
    starts[fi.nrec] = fi.n;
    /* the alignments kept: mapped, at least --min-mapq; in read order, their CIGARs side by side */
    uint64_t na = 0, nops = 0;
    alns = malloc((nr ? nr : 1) * sizeof *alns);
    bal = malloc(PILE_BATCH_ALNS * sizeof *bal);
    acoff = malloc((nr + 1) * 8);
    acig = malloc((coff[nr] ? coff[nr] : 1) * 4);
    if (!alns || !bal || !acoff || !acig) { fprintf(stderr, "out of memory\n"); goto done; }
    acoff[0] = 0;
    for (uint64_t i = 0; i < nr; i++) {
        const debwt_fm_hit *h = &hits[i];
        if ((h->flags & DEBWT_FM_MAP_UNMAPPED) || h->mapq < A->min_mapq) continue;
        alns[na].pattern = i; alns[na].tbeg = h->tbeg; alns[na].qbeg = h->qbeg;
        alns[na].strand = (h->flags & DEBWT_FM_MAP_REVERSE) ? 1 : 0;
        memcpy(acig + nops, cig + coff[i], (coff[i + 1] - coff[i]) * 4);
        nops += coff[i + 1] - coff[i];
        acoff[++na] = nops;
    }
    /* the positions walked: the whole text, or one region in extract's form */
    uint64_t gbeg = 0, gend = fi.n, r0 = 0, r1 = fi.nrec;
    if (A->region) {
        uint64_t rec = 0, beg = 0, end = 0;
        int whole = 0;
        if (parse_region(A->region, &rec, &beg, &end, &whole)) { fprintf(stderr, "--region: '%s' is not J or J:BEG-END\n", A->region); goto done; }
        const uint64_t len = rec < fi.nrec ? starts[rec + 1] - 1 - starts[rec] : 0;
        if (whole) end = len;
        if (rec >= fi.nrec || beg >= end || end > len) { fprintf(stderr, "--region: '%s' is empty or lies outside its record\n", A->region); goto done; }
        gbeg = starts[rec] + beg; gend = starts[rec] + end; r0 = rec; r1 = rec + 1;
    }
    const uint64_t W = A->window < gend - gbeg ? A->window : gend - gbeg;
    calls = malloc(W); refb = malloc(W);
    counts = consensus ? NULL : malloc(W * 32);
    if (!calls || !refb || (!consensus && !counts)) { fprintf(stderr, "out of memory\n"); goto done; }
    if (A->variants && !(vf = fopen(A->variants, "w"))) { fprintf(stderr, "cannot write %s\n", A->variants); goto done; }
    uint64_t vcap = 0, ecap = 0, ccap = 0, open_rec = ~0ull;
    for (uint64_t wb = gbeg; wb < gend; wb += W) {
        const uint64_t we = wb + W < gend ? wb + W : gend;
        for (uint64_t a0 = 0, first = 1; first || a0 < na; a0 += PILE_BATCH_ALNS, first = 0) {
            const uint64_t a1 = a0 + PILE_BATCH_ALNS < na ? a0 + PILE_BATCH_ALNS : na;
            const uint64_t p0 = a1 > a0 ? alns[a0].pattern : 0, p1 = a1 > a0 ? alns[a1 - 1].pattern + 1 : 0;
            for (uint64_t a = a0; a < a1; a++) { bal[a - a0] = alns[a]; bal[a - a0].pattern -= p0; }
            rc = debwt_fm_pileup(fm, seq, off + p0, p1 - p0, bal, a1 - a0, acoff + a0, acig, wb, we, first ? 0u : DEBWT_FM_PILE_ADD);
            if (rc) { fprintf(stderr, "%s\n", debwt_fm_last_error(fm)); goto done; }
        }
        uint64_t nv = 0;
        rc = debwt_fm_pile_call(fm, &A->call, calls, refb, vars, vcap, &nv);
        if (rc == DEBWT_ERANGE && nv > vcap) {
            free(vars);
            vars = malloc(nv * sizeof *vars);
            vcap = vars ? nv : 0;
            if (!vars) { fprintf(stderr, "out of memory\n"); goto done; }
            rc = debwt_fm_pile_call(fm, &A->call, calls, refb, vars, vcap, &nv);
        }
        if (rc) { fprintf(stderr, "%s\n", debwt_fm_last_error(fm)); goto done; }
        if (!consensus) {
            uint64_t win[2];
            rc = debwt_fm_pile_fetch(fm, win, counts, W);
            if (rc) { fprintf(stderr, "%s\n", debwt_fm_last_error(fm)); goto done; }
            uint64_t r = r0;
            for (uint64_t t = wb; t < we; t++) {
                const uint32_t *c = counts + (t - wb) * 8;
                const uint64_t d = (uint64_t)c[0] + c[1] + c[2] + c[3] + c[4];
                if (!d) continue;
                while (t >= starts[r + 1]) r++;
                printf("%llu\t%llu\t%c\t%llu\t%u\t%u\t%u\t%u\t%u\t%u\t%u\n", (unsigned long long)r, (unsigned long long)(t - starts[r] + 1),
                       "ACGTN"[refb[t - wb] > 4 ? 4 : refb[t - wb]], (unsigned long long)d, c[0], c[1], c[2], c[3], c[4], c[5], c[6]);
            }
            continue;
        }
        /* consensus: the insertions behind the flagged variants, voted; then the strings of this window */
        uint64_t nf = 0, nev = 0, nb = 0;
        for (uint64_t k = 0; k < nv; k++) nf += (vars[k].call & 0x10) != 0;
        free(vt); free(ioff); free(isup); free(idep); free(ibases);
        vt = malloc((nf ? nf : 1) * 8); ioff = malloc((nf + 1) * 8); isup = malloc((nf ? nf : 1) * 4); idep = malloc((nf ? nf : 1) * 4);
        ibases = NULL;
        if (!vt || !ioff || !isup || !idep) { fprintf(stderr, "out of memory\n"); goto done; }
        nf = 0;
        for (uint64_t k = 0; k < nv; k++)
            if (vars[k].call & 0x10) { vt[nf] = vars[k].t; idep[nf] = vars[k].depth; nf++; }
        if (nf) {
            rc = debwt_fm_pile_insertions(fm, nr, off, alns, na, acoff, acig, vt, nf, ev, ecap, &nev);
            if (rc == DEBWT_ERANGE && nev > ecap) {
                free(ev);
                ev = malloc(nev * sizeof *ev);
                ecap = ev ? nev : 0;
                if (!ev) { fprintf(stderr, "out of memory\n"); goto done; }
                rc = debwt_fm_pile_insertions(fm, nr, off, alns, na, acoff, acig, vt, nf, ev, ecap, &nev);
            }
            if (rc) { fprintf(stderr, "%s\n", debwt_fm_last_error(fm)); goto done; }
        }
        ioff[0] = 0;
        for (int pass = 0; pass < 2; pass++) {            /* the lengths of the voted strings, then the strings */
            uint64_t e0 = 0;
            for (uint64_t k = 0; k < nf; k++) {
                uint64_t e1 = e0, len = 0;
                while (e1 < nev && ev[e1].t == vt[k]) e1++;
                rc = debwt_fm_ins_vote(seq, off, nr, alns, na, ev + e0, e1 - e0, pass ? ibases + ioff[k] : NULL,
                                       pass ? ioff[k + 1] - ioff[k] : 0, &len, &isup[k]);
                if (rc && !(rc == DEBWT_ERANGE && !pass)) { fprintf(stderr, "the insertion vote failed\n"); goto done; }
                if (!pass) ioff[k + 1] = ioff[k] + len;
                e0 = e1;
            }
            if (!pass) {
                nb = ioff[nf];
                ibases = malloc(nb ? nb : 1);
                if (!ibases) { fprintf(stderr, "out of memory\n"); goto done; }
            }
        }
        rc = debwt_fm_consensus(refb, calls, wb, we, vt, ioff, ibases, isup, idep, nf, A->call.min_permille, starts, fi.nrec, fi.n,
                                ooff, cons, ccap);
        if (rc == DEBWT_ERANGE) {
            free(cons);
            ccap = ooff[fi.nrec];
            cons = malloc(ccap ? ccap : 1);
            if (!cons) { fprintf(stderr, "out of memory\n"); goto done; }
            rc = debwt_fm_consensus(refb, calls, wb, we, vt, ioff, ibases, isup, idep, nf, A->call.min_permille, starts, fi.nrec,
                                    fi.n, ooff, cons, ccap);
        }
        if (rc) { fprintf(stderr, "the consensus failed\n"); goto done; }
        for (uint64_t r = r0; r < r1; r++) {
            const uint64_t rs = starts[r], re = starts[r + 1] - 1;
            if (re <= wb || rs >= we) continue;           /* no base of the record in this window */
            if (open_rec != r) {
                if (open_rec != ~0ull) putchar('\n');
                if (A->region) printf(">%s\n", A->region); else printf(">%llu\n", (unsigned long long)r);
                open_rec = r;
            }
            fwrite(cons + ooff[r], 1, ooff[r + 1] - ooff[r], stdout);
        }
        if (vf) {
            uint64_t r = r0, kf = 0;
            for (uint64_t k = 0; k < nv; k++) {
                const debwt_fm_variant *v = &vars[k];
                while (v->t >= starts[r + 1]) r++;
                const uint32_t b = v->call & 15u;
                if (b != v->ref)
                    fprintf(vf, "%llu\t%llu\t%c\t%c\t%u\t%u\n", (unsigned long long)r, (unsigned long long)(v->t - starts[r] + 1),
                            "ACGT"[v->ref & 3], b == 4 ? '-' : "ACGT"[b & 3], v->depth, v->count);
                if (v->call & 0x10) {
                    fprintf(vf, "%llu\t%llu\t%c\t+", (unsigned long long)r, (unsigned long long)(v->t - starts[r] + 1), "ACGT"[v->ref & 3]);
                    fwrite(ibases + ioff[kf], 1, ioff[kf + 1] - ioff[kf], vf);
                    fprintf(vf, "\t%u\t%u\n", v->depth, isup[kf]);
                    kf++;
                }
            }
        }
    }
    if (consensus && open_rec != ~0ull) putchar('\n');
    ret = fflush(stdout) ? 1 : 0;
    if (vf && fflush(vf)) ret = 1;
done:
    if (vf) fclose(vf);
    debwt_free_packed(&pt);
    free(coff); free(cig); free(hits); free(info); free(starts); free(ooff); free(alns); free(bal); free(acoff); free(acig);
    free(counts); free(calls); free(refb); free(vars); free(ev); free(vt); free(ioff); free(isup); free(idep); free(ibases); free(cons);
    debwt_fm_destroy(fm);
    free(B.seq); free(B.off);
    free_patterns(&P); free_patterns(&M);
    return ret;
}

/* ---- kmers / correct -------------------------------------------------------------------------------------------------- */

static int cmd_kmers(const struct query_args *A) {
    struct patterns P;
    if (read_patterns(A->file, &P)) { free_patterns(&P); return 1; }
    debwt_fm *fm = NULL;
    if (open_index(A->out, A->device, &fm)) { free_patterns(&P); return 1; }
    int ret = 1;
    uint64_t total = 0, *coff = malloc((P.n + 1) * 8);
    for (uint64_t i = 0; i < P.n; i++) {
        uint64_t m = P.off[i + 1] - P.off[i];
        total += m >= A->ko.k ? m - A->ko.k + 1 : 0;
    }
    uint32_t *cnt = malloc((total ? total : 1) * 4);
    if (!coff || !cnt) { fprintf(stderr, "out of memory\n"); goto done; }
    int rc = debwt_fm_kmer_counts(fm, P.seq, P.off, P.n, A->ko.k, A->flags, coff, cnt, total);
    if (rc) { fprintf(stderr, "%s\n", debwt_fm_last_error(fm)); goto done; }
    for (uint64_t i = 0; i < P.n; i++) {
        printf("%s\t", P.name[i]);
        if (coff[i + 1] == coff[i]) putchar('*');
        for (uint64_t j = coff[i]; j < coff[i + 1]; j++) printf("%s%u", j > coff[i] ? "," : "", cnt[j]);
        putchar('\n');
    }
    ret = fflush(stdout) ? 1 : 0;
done:
    free(coff); free(cnt);
    free_patterns(&P);
    debwt_fm_destroy(fm);
    return ret;
}

static int cmd_correct(const struct query_args *A) {
    struct patterns P;
    if (read_patterns(A->file, &P)) { free_patterns(&P); return 1; }
    debwt_fm *fm = NULL;
    if (open_index(A->out, A->device, &fm)) { free_patterns(&P); return 1; }
    int ret = 1, rc;
    debwt_fm_correct_opts ko = A->ko, *o = &ko;
    char *fixed = malloc(P.len ? P.len : 1);
    debwt_fm_correct_info *info = malloc((P.n ? P.n : 1) * sizeof *info);
    FILE *rf = NULL;
    if (!fixed || !info) { fprintf(stderr, "out of memory\n"); goto done; }
    if (A->auto_count) {                                  /* the valley of the spectrum at this K and these strands */
        uint64_t hist[256];
        debwt_fm_spectrum_totals tot;
        debwt_fm_spectrum_summary sum;
        rc = debwt_fm_spectrum(fm, ko.k, ko.flags, 256, hist, &tot);
        if (rc) { fprintf(stderr, "%s\n", debwt_fm_last_error(fm)); goto done; }
        debwt_fm_spectrum_threshold(hist, 256, tot.total, &sum);
        if (!sum.valley) {
            fprintf(stderr, "correct: --min-count auto: the %u-mer spectrum of the collection has no valley\n", ko.k);
            goto done;
        }
        ko.min_count = (uint32_t)sum.valley;
        fprintf(stderr, "correct: --min-count auto: %u (the valley of the %u-mer spectrum, peak %llu)\n", ko.min_count, ko.k,
                (unsigned long long)sum.peak);
    }
    rc = debwt_fm_correct(fm, P.seq, P.off, P.n, o, fixed, info);
    if (rc) { fprintf(stderr, "%s\n", debwt_fm_last_error(fm)); goto done; }
    if (A->report && !(rf = fopen(A->report, "w"))) { fprintf(stderr, "cannot write %s\n", A->report); goto done; }
    for (uint64_t i = 0; i < P.n; i++) {
        printf(">%s\n", P.name[i]);
        fwrite(fixed + P.off[i], 1, P.off[i + 1] - P.off[i], stdout);
        putchar('\n');
        if (rf) {
            const uint32_t f = info[i].flags;
            fprintf(rf, "%s\t%s\t%u\t%u\t%u\n", P.name[i],
                    f & DEBWT_FM_CORRECT_SHORT ? "short" : f & DEBWT_FM_CORRECT_CLEAN ? "clean" : f & DEBWT_FM_CORRECT_FIXED ? "fixed" : "weak",
                    info[i].fixes, info[i].weak_before, info[i].weak_after);
        }
    }
    if (rf && fclose(rf)) { rf = NULL; fprintf(stderr, "cannot write %s\n", A->report); goto done; }
    rf = NULL;
    debwt_fm_correct_stats st;
    debwt_fm_correct_stats_get(fm, &st);
    fprintf(stderr, "correct: %llu reads, %llu short, %llu clean, %llu fixed, %llu weak; %llu fixes in %llu rounds, k = %u, %.1f ms\n",
            (unsigned long long)P.n, (unsigned long long)st.reads_short, (unsigned long long)st.reads_clean,
            (unsigned long long)st.reads_fixed, (unsigned long long)st.reads_weak, (unsigned long long)st.fixes,
            (unsigned long long)st.rounds, o->k, st.kmers.ms_wall);
    ret = fflush(stdout) ? 1 : 0;
done:
    if (rf) fclose(rf);
    free(fixed); free(info);
    free_patterns(&P);
    debwt_fm_destroy(fm);
    return ret;
}

/* ---- spectrum ---------------------------------------------------------------------------------------------------------- */

static int cmd_spectrum(const struct query_args *A) {
    const uint32_t k = A->ko.k, flags = A->ko.flags;
    debwt_fm *fm = NULL;
    if (open_index(A->out, A->device, &fm)) return 1;
    int ret = 1;
    uint64_t *hist = calloc(A->bins, 8), *codes = NULL, count = 0;
    uint32_t *mults = NULL;
    FILE *lf = NULL;
    debwt_fm_spectrum_totals tot;
    debwt_fm_spectrum_summary sum;
    if (!hist) { fprintf(stderr, "out of memory\n"); goto done; }
    int rc = debwt_fm_spectrum(fm, k, flags, A->bins, hist, &tot);
    if (rc) { fprintf(stderr, "%s\n", debwt_fm_last_error(fm)); goto done; }
    debwt_fm_spectrum_threshold(hist, A->bins, tot.total, &sum);
    printf("# k\t%u\n# strands\t%s\n# distinct\t%llu\n# total\t%llu\n# valley\t%llu\n# peak\t%llu\n# est_size\t%llu\n", k,
           flags & DEBWT_FM_BOTH_STRANDS ? "both" : "forward", (unsigned long long)tot.distinct, (unsigned long long)tot.total,
           (unsigned long long)sum.valley, (unsigned long long)sum.peak, (unsigned long long)sum.est_size);
    for (uint32_t c = 1; c < A->bins; c++)
        if (hist[c]) printf("%s%u\t%llu\n", c == A->bins - 1 ? ">=" : "", c, (unsigned long long)hist[c]);
    if (A->list) {
        rc = debwt_fm_kmer_list(fm, k, flags, A->at_least, A->at_most, NULL, NULL, 0, &count);
        if (rc && rc != DEBWT_ERANGE) { fprintf(stderr, "%s\n", debwt_fm_last_error(fm)); goto done; }
        codes = malloc((count ? count : 1) * 8); mults = malloc((count ? count : 1) * 4);
        if (!codes || !mults) { fprintf(stderr, "out of memory\n"); goto done; }
        if (count && (rc = debwt_fm_kmer_list(fm, k, flags, A->at_least, A->at_most, codes, mults, count, &count))) {
            fprintf(stderr, "%s\n", debwt_fm_last_error(fm));
            goto done;
        }
        if (!(lf = fopen(A->list, "w"))) { fprintf(stderr, "cannot write %s\n", A->list); goto done; }
        char w[33];
        w[k] = 0;
        for (uint64_t i = 0; i < count; i++) {
            for (uint32_t j = 0; j < k; j++) w[j] = "ACGT"[(codes[i] >> (2 * (k - 1 - j))) & 3];
            fprintf(lf, "%s\t%u\n", w, mults[i]);
        }
        if (fclose(lf)) { lf = NULL; fprintf(stderr, "cannot write %s\n", A->list); goto done; }
        lf = NULL;
    }
    debwt_fm_spectrum_stats st;
    debwt_fm_spectrum_stats_get(fm, &st);
    fprintf(stderr, "spectrum: k = %u, %s, %llu distinct, %llu in all; valley %llu, peak %llu, size about %llu%s; %.1f ms\n", k,
            flags & DEBWT_FM_BOTH_STRANDS ? "both strands" : "forward", (unsigned long long)tot.distinct,
            (unsigned long long)tot.total, (unsigned long long)sum.valley, (unsigned long long)sum.peak,
            (unsigned long long)sum.est_size, sum.valley ? "" : " (no valley)", st.ms_wall);
    ret = fflush(stdout) ? 1 : 0;
done:
    if (lf) fclose(lf);
    free(hist); free(codes); free(mults);
    debwt_fm_destroy(fm);
    return ret;
}

/* ---- lcp --------------------------------------------------------------------------------------------------------------- */

/* one kept array to a raw file, in pieces */
static int write_esa_array(debwt_fm *fm, int which, size_t width, uint64_t n, const char *path) {
    const uint64_t piece = 1ull << 22;
    void *buf = malloc((size_t)(n < piece ? (n ? n : 1) : piece) * width);
    FILE *f = fopen(path, "wb");
    int ret = 1;
    if (!buf) { fprintf(stderr, "out of memory\n"); goto done; }
    if (!f) { fprintf(stderr, "cannot write %s\n", path); goto done; }
    for (uint64_t lo = 0; lo < n; lo += piece) {
        const uint64_t cnt = n - lo < piece ? n - lo : piece;
        if (debwt_fm_esa_fetch(fm, which, lo, cnt, buf)) { fprintf(stderr, "%s\n", debwt_fm_last_error(fm)); goto done; }
        if (fwrite(buf, width, cnt, f) != cnt) { fprintf(stderr, "cannot write %s\n", path); goto done; }
    }
    ret = 0;
done:
    if (f && fclose(f)) { fprintf(stderr, "cannot write %s\n", path); ret = 1; }
    free(buf);
    return ret;
}

/* the record of text position p: the last start at or before it (starts: nrec entries, ascending) */
static uint64_t record_of(const uint64_t *starts, uint64_t nrec, uint64_t p) {
    uint64_t lo = 0, hi = nrec;
    while (hi - lo > 1) {
        const uint64_t mid = (lo + hi) >> 1;
        if (starts[mid] <= p) lo = mid; else hi = mid;
    }
    return lo;
}

static int cmd_lcp(const struct query_args *A) {
    debwt_fm *fm = NULL;
    if (open_index(A->out, A->device, &fm)) return 1;
    int ret = 1;
    debwt_fm_info fi;
    debwt_fm_info_get(fm, &fi);
    uint64_t *starts = malloc(fi.nrec * 8), *distinct = calloc(A->profile_k ? A->profile_k : 1, 8);
    debwt_fm_esa_summary sm;
    debwt_fm_esa_stats st;
    if (!starts || !distinct) { fprintf(stderr, "out of memory\n"); goto done; }
    if (debwt_fm_record_starts(fm, starts, fi.nrec) ||
        debwt_fm_esa_build(fm, A->max_lcp, (A->sa_file ? DEBWT_FM_ESA_SA : 0u) | (A->da_file ? DEBWT_FM_ESA_DA : 0u)) ||
        debwt_fm_esa_summary_get(fm, &sm) || (A->profile_k && debwt_fm_esa_profile(fm, A->profile_k, distinct))) {
        fprintf(stderr, "%s\n", debwt_fm_last_error(fm));
        goto done;
    }
    if (A->lcp_file && write_esa_array(fm, DEBWT_FM_ESA_LCP_ARRAY, 4, fi.n, A->lcp_file)) goto done;
    if (A->sa_file && write_esa_array(fm, DEBWT_FM_ESA_SA_ARRAY, 8, fi.n, A->sa_file)) goto done;
    if (A->da_file && write_esa_array(fm, DEBWT_FM_ESA_DA_ARRAY, 4, fi.n, A->da_file)) goto done;
    const uint64_t ra = record_of(starts, fi.nrec, sm.pos_prev), rb = record_of(starts, fi.nrec, sm.pos);
    printf("# n=%llu\tmax=%llu\tmax_row=%llu\tprev=%llu:%llu\tpos=%llu:%llu\tmean=%.6f\n", (unsigned long long)sm.n,
           (unsigned long long)sm.max, (unsigned long long)sm.max_row, (unsigned long long)ra,
           (unsigned long long)(sm.pos_prev - starts[ra]), (unsigned long long)rb, (unsigned long long)(sm.pos - starts[rb]),
           (double)sm.sum / (double)sm.n);
    for (uint32_t k = 1; k <= A->profile_k; k++) printf("%u\t%llu\n", k, (unsigned long long)distinct[k - 1]);
    debwt_fm_esa_stats_get(fm, &st);
    fprintf(stderr, "lcp: %llu rows, max %llu at row %llu, %llu capped; %llu chunks of %llu, %.2f symbols compared per position; "
                    "walk %.1f, scatter %.1f, plcp %.1f, rows %.1f ms, %.1f ms in all\n",
            (unsigned long long)sm.n, (unsigned long long)sm.max, (unsigned long long)sm.max_row, (unsigned long long)sm.capped,
            (unsigned long long)st.chunks, (unsigned long long)st.chunk_len, (double)st.symbols_compared / (double)sm.n,
            st.ms_walk, st.ms_scatter, st.ms_plcp, st.ms_rows, st.ms_wall);
    ret = fflush(stdout) ? 1 : 0;
done:
    free(starts); free(distinct);
    debwt_fm_destroy(fm);
    return ret;
}

/* ---- repeats ----------------------------------------------------------------------------------------------------------- */

static int cmd_repeats(const struct query_args *A) {
    const int mums = A->cmd == CMD_MUMS;
    debwt_fm *fm = NULL;
    if (open_index(A->out, A->device, &fm)) return 1;
    int ret = 1, rc;
    debwt_fm_info fi;
    debwt_fm_info_get(fm, &fi);
    uint64_t *starts = malloc(fi.nrec * 8), *sa = malloc(fi.n * 8), *off = NULL, count = 0;
    debwt_fm_repeat *rp = NULL;
    debwt_fm_extract_job *jb = NULL;
    char *bases = NULL;
    uint64_t bcap = 0;
    debwt_fm_repeat_opts o = {A->min_len, A->kind, A->min_occ, A->max_occ};
    debwt_fm_record_filter flt = {A->min_records ? A->min_records : 1, A->max_records, A->unique ? DEBWT_FM_RECORDS_UNIQUE : 0u, 0};
    const int by_record = A->by_record || mums;
    uint32_t *nrecs = NULL;
    struct occ *oc = NULL;
    debwt_fm_repeat_stats st;
    if (mums) {                                                 /* maximal, once in each of at least q records, nowhere else */
        flt.min_records = A->min_records ? A->min_records : fi.nrec;
        flt.flags = DEBWT_FM_RECORDS_UNIQUE;
        o.kind = DEBWT_FM_REPEAT_MAXIMAL; o.min_occ = flt.min_records > 2 ? flt.min_records : 2; o.max_occ = 0;
    }
    if (!starts || !sa) { fprintf(stderr, "out of memory\n"); goto done; }
    if (debwt_fm_record_starts(fm, starts, fi.nrec) ||
        debwt_fm_esa_build(fm, A->max_lcp, DEBWT_FM_ESA_SA | (by_record ? DEBWT_FM_ESA_DA : 0u)) ||
        (by_record && debwt_fm_records_build(fm))) {
        fprintf(stderr, "%s\n", debwt_fm_last_error(fm));
        goto done;
    }
    rc = by_record ? debwt_fm_repeats_records(fm, &o, &flt, NULL, NULL, 0, &count) : debwt_fm_repeats(fm, &o, NULL, 0, &count);
    if (rc && rc != DEBWT_ERANGE) { fprintf(stderr, "%s\n", debwt_fm_last_error(fm)); goto done; }
    rp = malloc((count ? count : 1) * sizeof *rp);
    if (by_record) nrecs = malloc((count ? count : 1) * sizeof *nrecs);
    if (!rp || (by_record && !nrecs)) { fprintf(stderr, "out of memory\n"); goto done; }
    if (count && (by_record ? debwt_fm_repeats_records(fm, &o, &flt, rp, nrecs, count, &count) : debwt_fm_repeats(fm, &o, rp, count, &count))) {
        fprintf(stderr, "%s\n", debwt_fm_last_error(fm));
        goto done;
    }
    debwt_fm_repeat_stats_get(fm, &st);
    for (uint64_t lo = 0; lo < fi.n; lo += 1ull << 22) {
        const uint64_t cnt = fi.n - lo < (1ull << 22) ? fi.n - lo : (1ull << 22);
        if (debwt_fm_esa_fetch(fm, DEBWT_FM_ESA_SA_ARRAY, lo, cnt, sa + lo)) { fprintf(stderr, "%s\n", debwt_fm_last_error(fm)); goto done; }
    }
    if (mums)
        printf("# mums=%llu\tmin_records=%llu\tlongest=%llu\n", (unsigned long long)st.reported, (unsigned long long)flt.min_records,
               (unsigned long long)st.longest_len);
    else
        printf("# intervals=%llu\tmaximal=%llu\tsupermaximal=%llu\treported=%llu\tlongest=%llu\n", (unsigned long long)st.intervals,
               (unsigned long long)st.maximal, (unsigned long long)st.supermaximal, (unsigned long long)st.reported,
               (unsigned long long)st.longest_len);
    if (mums) {
        oc = malloc((fi.nrec ? fi.nrec : 1) * sizeof *oc);      /* unique: a multi-MUM has at most one occurrence per record */
        if (!oc) { fprintf(stderr, "out of memory\n"); goto done; }
    }
    if (A->seq) {
        off = malloc((EXTRACT_BATCH_JOBS + 1) * 8);
        jb = malloc(EXTRACT_BATCH_JOBS * sizeof *jb);
        if (!off || !jb) { fprintf(stderr, "out of memory\n"); goto done; }
        if (fi.nrec >> 32) { fprintf(stderr, "repeats --seq: 2^32 records or more\n"); goto done; }
    }
    for (uint64_t j0 = 0; j0 < count;) {
        uint64_t j1 = j0, bytes = 0;
        while (j1 < count && j1 - j0 < EXTRACT_BATCH_JOBS) {      /* at least one repeat, however long */
            if (j1 > j0 && bytes + rp[j1].len > EXTRACT_BATCH_BYTES) break;
            if (A->seq) {
                const uint64_t p = sa[rp[j1].row_lo], r = record_of(starts, fi.nrec, p);
                jb[j1 - j0].record = (uint32_t)r; jb[j1 - j0].reserved = 0; jb[j1 - j0].offset = p - starts[r]; jb[j1 - j0].length = rp[j1].len;
            }
            bytes += rp[j1].len; j1++;
        }
        if (A->seq) {
            if (bytes > bcap) {
                free(bases);
                bases = malloc(bytes);
                bcap = bases ? bytes : 0;
                if (!bases) { fprintf(stderr, "out of memory\n"); goto done; }
            }
            if (debwt_fm_extract(fm, jb, j1 - j0, off, bases, bcap)) { fprintf(stderr, "%s\n", debwt_fm_last_error(fm)); goto done; }
        }
        for (uint64_t j = j0; j < j1; j++) {
            const debwt_fm_repeat *x = &rp[j];
            const uint64_t p = sa[x->row_lo], r = record_of(starts, fi.nrec, p);
            if (mums) {                                         /* len, then the occurrence in every record, ascending by record */
                if (x->count > fi.nrec) { fprintf(stderr, "mums: more occurrences than records\n"); goto done; }
                for (uint64_t t = 0; t < x->count; t++) {
                    const uint64_t q = sa[x->row_lo + t], rq = record_of(starts, fi.nrec, q);
                    oc[t].rec = rq; oc[t].off = q - starts[rq]; oc[t].strand = 0; oc[t].mm = 0;
                }
                qsort(oc, x->count, sizeof *oc, cmp_occ);
                printf("%u", x->len);
                for (uint64_t t = 0; t < x->count; t++)
                    printf("%c%llu:%llu", t ? ',' : '\t', (unsigned long long)oc[t].rec, (unsigned long long)oc[t].off);
                if (A->seq) { putchar('\t'); fwrite(bases + off[j - j0], 1, off[j - j0 + 1] - off[j - j0], stdout); }
                putchar('\n');
                continue;
            }
            printf("%u\t%llu\t", x->len, (unsigned long long)x->count);
            if (by_record) printf("%u\t", nrecs[j]);
            printf("%c\t%llu,%llu,%llu,%llu,%llu\t%llu:%llu",
                   x->flags & DEBWT_FM_REPEAT_IS_SUPERMAXIMAL ? 'S' : x->flags & DEBWT_FM_REPEAT_IS_MAXIMAL ? 'M' : '-',
                   (unsigned long long)x->left[0], (unsigned long long)x->left[1], (unsigned long long)x->left[2],
                   (unsigned long long)x->left[3], (unsigned long long)x->left[4], (unsigned long long)r,
                   (unsigned long long)(p - starts[r]));
            if (A->seq) { putchar('\t'); fwrite(bases + off[j - j0], 1, off[j - j0 + 1] - off[j - j0], stdout); }
            if (A->occurrences)
                for (uint64_t t = 0; t < x->count; t++) {
                    const uint64_t q = sa[x->row_lo + t], rq = record_of(starts, fi.nrec, q);
                    printf("%c%llu:%llu", t ? ',' : '\t', (unsigned long long)rq, (unsigned long long)(q - starts[rq]));
                }
            putchar('\n');
        }
        j0 = j1;
    }
    fprintf(stderr, "repeats: %llu rows, %llu intervals of at least %u bases (%llu maximal, %llu supermaximal, %llu capped), %llu "
                    "reported, longest %llu; %llu levels of fanout %llu, %.2f reads per row searched; tree %.1f, search %.1f, "
                    "write %.1f ms\n",
            (unsigned long long)st.rows, (unsigned long long)st.intervals, A->min_len, (unsigned long long)st.maximal,
            (unsigned long long)st.supermaximal, (unsigned long long)st.capped_intervals, (unsigned long long)st.reported,
            (unsigned long long)st.longest_len, (unsigned long long)st.levels, (unsigned long long)st.fanout,
            st.searched ? (double)st.search_steps / (double)st.searched : 0.0, st.ms_tree, st.ms_search, st.ms_write);
    ret = fflush(stdout) ? 1 : 0;
done:
    free(starts); free(sa); free(rp); free(off); free(jb); free(bases); free(nrecs); free(oc);
    debwt_fm_destroy(fm);
    return ret;
}

/* ---- dbg ------------------------------------------------------------------------------------------------------------------ */

static int cmp_u64_desc(const void *a, const void *b) {
    const uint64_t x = *(const uint64_t *)a, y = *(const uint64_t *)b;
    return x < y ? 1 : x > y ? -1 : 0;
}

/* the largest L such that the strings of length >= L hold at least half of all bases; 0 without strings.  Sorts len. */
static uint64_t n50_of(uint64_t *len, uint64_t count) {
    uint64_t total = 0, run = 0;
    for (uint64_t i = 0; i < count; i++) total += len[i];
    qsort(len, count, sizeof *len, cmp_u64_desc);
    for (uint64_t i = 0; i < count; i++) {
        run += len[i];
        if (run >= total - run) return len[i];
    }
    return 0;
}

/* the compacted de Bruijn graph of the collection's k-mers (Definition 13), as GFA 1 or as FASTA */
static int cmd_dbg(const struct query_args *A) {
    const uint32_t k = A->ko.k;
    debwt_fm *fm = NULL;
    if (open_index(A->out, A->device, &fm)) return 1;
    int ret = 1, rc;
    debwt_fm_cdbg_sizes sz = {0, 0, 0};
    debwt_fm_unitig *un = NULL;
    debwt_fm_cdbg_edge *ed = NULL;
    uint8_t *seq = NULL;
    uint64_t *len = NULL;
    debwt_fm_cdbg_stats st;
    if (debwt_fm_esa_build(fm, k + 1, DEBWT_FM_ESA_SA | DEBWT_FM_ESA_DA)) {   /* the call tells lcp = k from lcp > k, no more */
        fprintf(stderr, "%s\n", debwt_fm_last_error(fm));
        goto done;
    }
    rc = debwt_fm_cdbg(fm, k, 0, NULL, 0, NULL, 0, NULL, 0, &sz);
    if (rc && rc != DEBWT_ERANGE) { fprintf(stderr, "%s\n", debwt_fm_last_error(fm)); goto done; }
    un = malloc((sz.unitigs ? sz.unitigs : 1) * sizeof *un);
    ed = malloc((sz.edges ? sz.edges : 1) * sizeof *ed);
    seq = malloc(sz.seq_bytes ? sz.seq_bytes : 1);
    len = malloc((sz.unitigs ? sz.unitigs : 1) * sizeof *len);
    if (!un || !ed || !seq || !len) { fprintf(stderr, "out of memory\n"); goto done; }
    if (sz.unitigs && debwt_fm_cdbg(fm, k, 0, un, sz.unitigs, seq, sz.seq_bytes, ed, sz.edges, &sz)) {
        fprintf(stderr, "%s\n", debwt_fm_last_error(fm));
        goto done;
    }
    debwt_fm_cdbg_stats_get(fm, &st);
    if (!A->fasta) printf("H\tVN:Z:1.0\n");
    for (uint64_t u = 0; u < sz.unitigs; u++) {
        const uint64_t m = (uint64_t)un[u].nodes + k - 1;
        const int circular = (un[u].flags & DEBWT_FM_CDBG_CIRCULAR) != 0;
        len[u] = m;
        if (A->fasta) printf(">u%llu nodes=%u kc=%llu%s\n", (unsigned long long)u, un[u].nodes, (unsigned long long)un[u].kmer_count, circular ? " circular" : "");
        else printf("S\t%llu\t", (unsigned long long)u);
        fwrite(seq + un[u].seq_offset, 1, m, stdout);
        if (A->fasta) putchar('\n');
        else printf("\tLN:i:%llu\tKC:i:%llu%s\n", (unsigned long long)m, (unsigned long long)un[u].kmer_count, circular ? "\tCL:Z:circular" : "");
    }
    if (!A->fasta)
        for (uint64_t e = 0; e < sz.edges; e++) printf("L\t%u\t+\t%u\t+\t%uM\n", ed[e].from, ed[e].to, k - 1);
    {
        uint64_t longest = 0;
        for (uint64_t u = 0; u < sz.unitigs; u++) longest = len[u] > longest ? len[u] : longest;
        fprintf(stderr, "# dbg\tk=%u\tnodes=%llu\tunitigs=%llu\tcircular=%llu\tedges=%llu\tlongest=%llu\tN50=%llu\trounds=%llu\t"
                        "nodes %.1f, links %.1f, rank %.1f, write %.1f ms\n",
                k, (unsigned long long)st.nodes, (unsigned long long)sz.unitigs, (unsigned long long)st.circular,
                (unsigned long long)sz.edges, (unsigned long long)longest, (unsigned long long)n50_of(len, sz.unitigs),
                (unsigned long long)st.jump_rounds, st.ms_nodes, st.ms_links, st.ms_rank, st.ms_write);
    }
    ret = fflush(stdout) ? 1 : 0;
done:
    free(un); free(ed); free(seq); free(len);
    debwt_fm_destroy(fm);
    return ret;
}

/* the compacted de Bruijn graph over both strands (Definition 14), as GFA 1 or as FASTA: cmd_dbg with oriented edge ends */
static int cmd_bidbg(const struct query_args *A) {
    const uint32_t k = A->ko.k;
    if (!(k & 1u)) { fprintf(stderr, "-k: bidbg takes an odd k-mer length (an even one can be its own reverse complement)\n"); return 1; }
    debwt_fm *fm = NULL;
    if (open_index(A->out, A->device, &fm)) return 1;
    int ret = 1, rc;
    debwt_fm_cdbg_sizes sz = {0, 0, 0};
    debwt_fm_unitig *un = NULL;
    debwt_fm_cdbg_edge *ed = NULL;
    uint8_t *seq = NULL;
    uint64_t *len = NULL;
    debwt_fm_cdbg_both_stats st;
    if (debwt_fm_esa_build(fm, k + 1, DEBWT_FM_ESA_SA | DEBWT_FM_ESA_DA)) {   /* the call tells lcp = k from lcp > k, no more */
        fprintf(stderr, "%s\n", debwt_fm_last_error(fm));
        goto done;
    }
    rc = debwt_fm_cdbg_both(fm, k, 0, NULL, 0, NULL, 0, NULL, 0, &sz);
    if (rc && rc != DEBWT_ERANGE) { fprintf(stderr, "%s\n", debwt_fm_last_error(fm)); goto done; }
    un = malloc((sz.unitigs ? sz.unitigs : 1) * sizeof *un);
    ed = malloc((sz.edges ? sz.edges : 1) * sizeof *ed);
    seq = malloc(sz.seq_bytes ? sz.seq_bytes : 1);
    len = malloc((sz.unitigs ? sz.unitigs : 1) * sizeof *len);
    if (!un || !ed || !seq || !len) { fprintf(stderr, "out of memory\n"); goto done; }
    if (sz.unitigs && debwt_fm_cdbg_both(fm, k, 0, un, sz.unitigs, seq, sz.seq_bytes, ed, sz.edges, &sz)) {
        fprintf(stderr, "%s\n", debwt_fm_last_error(fm));
        goto done;
    }
    debwt_fm_cdbg_both_stats_get(fm, &st);
    if (!A->fasta) printf("H\tVN:Z:1.0\n");
    for (uint64_t u = 0; u < sz.unitigs; u++) {
        const uint64_t m = (uint64_t)un[u].nodes + k - 1;
        const int circular = (un[u].flags & DEBWT_FM_CDBG_CIRCULAR) != 0;
        len[u] = m;
        if (A->fasta) printf(">u%llu nodes=%u kc=%llu%s\n", (unsigned long long)u, un[u].nodes, (unsigned long long)un[u].kmer_count, circular ? " circular" : "");
        else printf("S\t%llu\t", (unsigned long long)u);
        fwrite(seq + un[u].seq_offset, 1, m, stdout);
        if (A->fasta) putchar('\n');
        else printf("\tLN:i:%llu\tKC:i:%llu%s\n", (unsigned long long)m, (unsigned long long)un[u].kmer_count, circular ? "\tCL:Z:circular" : "");
    }
    if (!A->fasta)
        for (uint64_t e = 0; e < sz.edges; e++)
            printf("L\t%u\t%c\t%u\t%c\t%uM\n", ed[e].from >> 1, ed[e].from & 1u ? '-' : '+', ed[e].to >> 1, ed[e].to & 1u ? '-' : '+', k - 1);
    {
        uint64_t longest = 0;
        for (uint64_t u = 0; u < sz.unitigs; u++) longest = len[u] > longest ? len[u] : longest;
        fprintf(stderr, "# bidbg\tk=%u\tnodes=%llu\tunitigs=%llu\tcircular=%llu\tedges=%llu\thairpins=%llu\tlongest=%llu\tN50=%llu\t"
                        "rounds=%llu\tnodes %.1f, mates %.1f, links %.1f, rank %.1f, write %.1f ms\n",
                k, (unsigned long long)st.nodes, (unsigned long long)sz.unitigs, (unsigned long long)st.circular,
                (unsigned long long)sz.edges, (unsigned long long)st.hairpins, (unsigned long long)longest,
                (unsigned long long)n50_of(len, sz.unitigs), (unsigned long long)st.jump_rounds, st.ms_nodes, st.ms_mates,
                st.ms_links, st.ms_rank, st.ms_write);
    }
    ret = fflush(stdout) ? 1 : 0;
done:
    free(un); free(ed); free(seq); free(len);
    debwt_fm_destroy(fm);
    return ret;
}

/* ---- graph / unitigs --------------------------------------------------------------------------------------------------- */

/* the mirror of oriented node v of the both-strand graph: v ^ 1, or v itself for the one node of a self-rc read */
static uint32_t mirror_node(const uint8_t *state, uint32_t v) {
    return state[v & ~1u] == 0 && state[v | 1u] == 1 ? v : v ^ 1u;
}

static int cmd_graph(const struct query_args *A) {
    const int want_unitigs = A->cmd == CMD_UNITIGS, both = A->both;
    const debwt_fm_clean_opts *clean = A->clean ? &A->cl : NULL;
    debwt_fm *fm = NULL;
    if (open_index(A->out, A->device, &fm)) return 1;
    int ret = 1, rc = 0;
    debwt_fm_info fi;
    debwt_fm_info_get(fm, &fi);
    const uint64_t nrec = fi.nrec, nn = both ? 2 * nrec : nrec;       /* nodes: records, or 2r + o with --both-strands */
    uint64_t *starts = malloc((nrec + 1) * 8), *eoff = malloc((nn + 1) * 8), *uoff = malloc((nn + 1) * 8), *boff = NULL;
    uint8_t *state = malloc(nn ? nn : 1), *circ = malloc(nn ? nn : 1);
    uint32_t *mem = malloc((nn ? nn : 1) * 4);
    debwt_fm_edge *edges = NULL;
    debwt_fm_extract_job *jobs = NULL;
    char *bases = NULL;
    FILE *sf = NULL;
    if (!starts || !eoff || !uoff || !state || !circ || !mem) { fprintf(stderr, "out of memory\n"); goto done; }
    rc = debwt_fm_record_starts(fm, starts, nrec);
    if (rc) { fprintf(stderr, "%s\n", debwt_fm_last_error(fm)); goto done; }
    starts[nrec] = fi.n;                                  /* record r holds starts[r + 1] - 1 - starts[r] bases */
    const uint32_t flags = A->all_edges ? DEBWT_FM_GRAPH_ALL_EDGES : 0u;
    uint64_t cap = 4 * nn + 16;                           /* first estimate; the exact count on DEBWT_ERANGE */
    for (;;) {
        free(edges);
        edges = malloc(cap * sizeof *edges);
        if (!edges) { fprintf(stderr, "out of memory\n"); goto done; }
        rc = both ? debwt_fm_string_graph_both(fm, A->min_overlap, flags, state, eoff, edges, cap)
                  : debwt_fm_string_graph(fm, A->min_overlap, flags, state, eoff, edges, cap);
        if (rc == DEBWT_ERANGE && eoff[nn] > cap) { cap = eoff[nn]; continue; }
        break;
    }
    if (rc) { fprintf(stderr, "%s\n", debwt_fm_last_error(fm)); goto done; }
    if (clean) {                                          /* the states get clipped and popped, the edges at them go */
        debwt_fm_clean_opts co = *clean;
        co.flags = both ? DEBWT_FM_CLEAN_MIRRORED : 0u;
        uint8_t *keep = malloc(eoff[nn] ? eoff[nn] : 1);
        if (!keep) { fprintf(stderr, "out of memory\n"); goto done; }
        rc = debwt_fm_graph_clean(fm, state, eoff, edges, nn, &co, state, keep);
        if (!rc) rc = debwt_fm_edges_compact(eoff, edges, keep, nn, eoff, edges) ? DEBWT_EINTERNAL : 0;
        free(keep);
        if (rc) { fprintf(stderr, "%s\n", debwt_fm_last_error(fm)); goto done; }
    }
    if (A->states) {
        if (!(sf = fopen(A->states, "w"))) { fprintf(stderr, "cannot write %s\n", A->states); goto done; }
        for (uint64_t i = 0; i < nrec; i++) {
            const uint8_t x = state[both ? 2 * i : i];        /* per read: the state of its first node */
            fprintf(sf, "%llu\t%s\n", (unsigned long long)i, x == 0 ? "kept" : x == 1 ? "duplicate" : x == 2 ? "contained" : x == DEBWT_FM_NODE_CLIPPED ? "clipped" : "popped");
        }
        if (fclose(sf)) { sf = NULL; fprintf(stderr, "cannot write %s\n", A->states); goto done; }
        sf = NULL;
    }
    debwt_fm_graph_stats st;
    debwt_fm_graph_stats_get(fm, &st);
    if (both) {
        debwt_fm_graph_both_stats bs;
        debwt_fm_graph_both_stats_get(fm, &bs);
        st.kept = bs.kept; st.duplicates = bs.duplicates; st.contained = bs.contained;
        st.edges = bs.edges; st.reducible = bs.reducible; st.ms_wall = bs.ms_wall;
    }
    if (clean) {
        debwt_fm_clean_stats cs;
        debwt_fm_clean_stats_get(fm, &cs);
        fprintf(stderr, "clean: %llu rounds, %llu tips of %llu nodes clipped, %llu branches of %llu nodes popped; %llu edges left, %.1f ms\n",
                (unsigned long long)cs.rounds, (unsigned long long)cs.tips, (unsigned long long)cs.tip_nodes,
                (unsigned long long)cs.bubbles, (unsigned long long)cs.bubble_nodes, (unsigned long long)eoff[nn], cs.ms_wall);
    }
    uint64_t written = eoff[nn];
    if (!want_unitigs) {
        printf("H\tVN:Z:1.0\n");
        for (uint64_t i = 0; i < nrec; i++)
            if (state[both ? 2 * i : i] == 0)
                printf("S\t%llu\t*\tLN:i:%llu\n", (unsigned long long)i, (unsigned long long)(starts[i + 1] - 1 - starts[i]));
        for (uint64_t i = 0; i < nn; i++)
            for (uint64_t e = eoff[i]; e < eoff[i + 1]; e++) {
                if (!both) { printf("L\t%llu\t+\t%u\t+\t%uM\n", (unsigned long long)i, edges[e].record, edges[e].length); continue; }
                /* u -> v and its mirror v' -> u' are one GFA link: the lower of the two pairs is written */
                const uint32_t u = (uint32_t)i, v = edges[e].record, mv = mirror_node(state, v), mu = mirror_node(state, u);
                if (u > mv || (u == mv && v > mu)) { written--; continue; }
                printf("L\t%u\t%c\t%u\t%c\t%uM\n", u >> 1, u & 1 ? '-' : '+', v >> 1, v & 1 ? '-' : '+', edges[e].length);
            }
        fprintf(stderr, "graph: %llu records, %llu kept, %llu duplicates, %llu contained; %llu edges, %llu reducible, %llu written, %.1f ms\n",
                (unsigned long long)nrec, (unsigned long long)st.kept, (unsigned long long)st.duplicates,
                (unsigned long long)st.contained, (unsigned long long)st.edges, (unsigned long long)st.reducible,
                (unsigned long long)written, st.ms_wall);
        ret = fflush(stdout) ? 1 : 0;
        goto done;
    }
    uint64_t nu = 0;
    rc = both ? debwt_fm_unitigs_both(state, eoff, edges, nn, uoff, mem, circ, &nu)
              : debwt_fm_unitigs(state, eoff, edges, nrec, uoff, mem, circ, &nu);
    if (rc) { fprintf(stderr, "unitigs: the graph is inconsistent\n"); goto done; }
    /* every member but the last gives its first |S| - L_next bases; the last of a circular unitig is cut as well.  With
     * --both-strands a member 2r + 1 gives those of rc S_r: the last |S| - L_next bases of S_r, reverse-complemented below */
    const uint64_t nm = uoff[nu];
    jobs = malloc((nm ? nm : 1) * sizeof *jobs);
    boff = malloc((nm + 1) * 8);
    if (!jobs || !boff) { fprintf(stderr, "out of memory\n"); goto done; }
    uint64_t total = 0, longest = 0;
    for (uint64_t u = 0; u < nu; u++)
        for (uint64_t x = uoff[u]; x < uoff[u + 1]; x++) {
            const uint32_t v = mem[x], r = both ? v >> 1 : v;
            uint64_t len = starts[r + 1] - 1 - starts[r], cut = 0;
            if (x + 1 < uoff[u + 1] || circ[u]) cut = edges[eoff[v]].length;       /* a link's source has one out-edge */
            len -= cut;
            jobs[x].record = r; jobs[x].reserved = 0; jobs[x].offset = both && (v & 1) ? cut : 0; jobs[x].length = len;
            total += len;
        }
    bases = malloc(total ? total : 1);
    if (!bases) { fprintf(stderr, "out of memory\n"); goto done; }
    rc = debwt_fm_extract(fm, jobs, nm, boff, bases, total);
    if (rc) { fprintf(stderr, "%s\n", debwt_fm_last_error(fm)); goto done; }
    for (uint64_t x = 0; both && x < nm; x++) {
        if (!(mem[x] & 1)) continue;
        char *lo = bases + boff[x], *hi = bases + boff[x + 1];
        while (lo < hi) {                                     /* in place; the middle base of an odd length meets itself */
            const char a = *lo, b = *--hi;
            *lo++ = b == 'A' ? 'T' : b == 'C' ? 'G' : b == 'G' ? 'C' : 'A';
            if (lo <= hi) *hi = a == 'A' ? 'T' : a == 'C' ? 'G' : a == 'G' ? 'C' : 'A';
        }
    }
    for (uint64_t u = 0; u < nu; u++) {
        const uint64_t a = boff[uoff[u]], b = boff[uoff[u + 1]];
        if (b - a > longest) longest = b - a;
        if (both)
            printf(">unitig_%llu reads=%llu len=%llu circular=%u first=%u%c\n", (unsigned long long)u,
                   (unsigned long long)(uoff[u + 1] - uoff[u]), (unsigned long long)(b - a), circ[u], mem[uoff[u]] >> 1,
                   mem[uoff[u]] & 1 ? '-' : '+');
        else
            printf(">unitig_%llu reads=%llu len=%llu circular=%u first=%u\n", (unsigned long long)u,
                   (unsigned long long)(uoff[u + 1] - uoff[u]), (unsigned long long)(b - a), circ[u], mem[uoff[u]]);
        fwrite(bases + a, 1, b - a, stdout);
        putchar('\n');
    }
    fprintf(stderr, "unitigs: %llu records, %llu kept; %llu edges, %llu irreducible; %llu unitigs, %llu bases, the longest %llu\n",
            (unsigned long long)nrec, (unsigned long long)st.kept, (unsigned long long)st.edges,
            (unsigned long long)eoff[nn], (unsigned long long)nu, (unsigned long long)total, (unsigned long long)longest);
    ret = fflush(stdout) ? 1 : 0;
done:
    if (sf) fclose(sf);
    free(starts); free(eoff); free(uoff); free(boff); free(state); free(circ); free(mem); free(edges); free(jobs); free(bases);
    debwt_fm_destroy(fm);
    return ret;
}

/* ---- the command line -------------------------------------------------------------------------------------------------- */

/* what a command checks across its options before it runs, and which of its forms runs */
static int run_count(const struct query_args *A) {                          /* count, locate */
    if (A->search && A->count_records) { fprintf(stderr, "--records: only with exact patterns on one strand\n"); return 1; }
    return A->search ? cmd_search(A) : cmd_query(A);
}

static int run_overlaps(const struct query_args *A) {
    if (A->permille_given && !A->ovl_mm) { fprintf(stderr, "--max-error-permille: only with --max-mismatches\n"); usage(); return 1; }
    return cmd_overlaps(A);
}

static int run_map(const struct query_args *A) {                            /* map, pileup, consensus */
    if (!A->ref) fprintf(stderr, "%s: no --ref INPUT.fa[.gz]: the text is restored from %s.sa and the BWT\n", A->name, A->out);
    if (A->gap_given && !A->chain) { fprintf(stderr, "--max-gap: only with --chain\n"); return 1; }
    if (A->mate && A->chain) { fprintf(stderr, "--mate: not with --chain (pairs are mapped with the fixed band)\n"); return 1; }
    if (A->insert_given && !A->mate) { fprintf(stderr, "--insert: only with --mate\n"); return 1; }
    if (A->no_rescue && !A->mate) { fprintf(stderr, "--no-rescue: only with --mate\n"); return 1; }
    return A->cmd != CMD_MAP ? cmd_pile(A) : A->mate ? cmd_map_pairs(A) : cmd_map(A);
}

static int run_spectrum(const struct query_args *A) {
    if (A->filter_given && !A->list) { fprintf(stderr, "--at-least, --at-most: only with --list\n"); return 1; }
    if (A->at_least > A->at_most) { fprintf(stderr, "--at-least: above --at-most\n"); return 1; }
    return cmd_spectrum(A);
}

static int run_lcp(const struct query_args *A) {
    if (A->max_lcp && A->profile_k > A->max_lcp) { fprintf(stderr, "--profile: above --max-lcp\n"); return 1; }
    return cmd_lcp(A);
}

static int run_repeats(const struct query_args *A) {                        /* repeats, mums */
    if (A->max_occ && A->max_occ < A->min_occ) { fprintf(stderr, "--max-occ: below --min-occ\n"); return 1; }
    if (A->max_records && A->max_records < A->min_records) { fprintf(stderr, "--max-records: below --min-records\n"); return 1; }
    if (A->max_lcp && A->min_len >= A->max_lcp) { fprintf(stderr, "--min-len: not below --max-lcp (repeats of the capped length are not listed)\n"); return 1; }
    return cmd_repeats(A);
}

static int run_graph(const struct query_args *A) {                          /* graph, unitigs */
    if (A->clean && A->all_edges) { usage(); return 1; }
    if (A->clean && !A->cl.max_tip && !A->cl.max_bubble) { fprintf(stderr, "--clean: --max-tip and --max-bubble are both 0\n"); return 1; }
    return cmd_graph(A);
}

/* one row per subcommand.  file: the argument that is no option; maps: the command maps reads first and takes map's options */
enum file_rule { FILE_NEEDED, FILE_NONE, FILE_OR_ALL };                     /* FILE_OR_ALL: exactly one of --all and REGIONS */
static const struct command {
    const char *name; enum cmd cmd; enum file_rule file; int need_k, maps;
    int (*run)(const struct query_args *);
} commands[] = {
    {"index",     CMD_INDEX,     FILE_NEEDED, 0, 0, cmd_index},
    {"count",     CMD_COUNT,     FILE_NEEDED, 0, 0, run_count},
    {"locate",    CMD_LOCATE,    FILE_NEEDED, 0, 0, run_count},
    {"mems",      CMD_MEMS,      FILE_NEEDED, 0, 0, cmd_mems},
    {"map",       CMD_MAP,       FILE_NEEDED, 0, 1, run_map},
    {"pileup",    CMD_PILEUP,    FILE_NEEDED, 0, 1, run_map},
    {"consensus", CMD_CONSENSUS, FILE_NEEDED, 0, 1, run_map},
    {"overlaps",  CMD_OVERLAPS,  FILE_NEEDED, 0, 0, run_overlaps},
    {"extract",   CMD_EXTRACT,   FILE_OR_ALL, 0, 0, cmd_extract},
    {"kmers",     CMD_KMERS,     FILE_NEEDED, 1, 0, cmd_kmers},
    {"correct",   CMD_CORRECT,   FILE_NEEDED, 1, 0, cmd_correct},
    {"spectrum",  CMD_SPECTRUM,  FILE_NONE,   1, 0, run_spectrum},
    {"lcp",       CMD_LCP,       FILE_NONE,   0, 0, run_lcp},
    {"repeats",   CMD_REPEATS,   FILE_NONE,   0, 0, run_repeats},
    {"mums",      CMD_MUMS,      FILE_NONE,   0, 0, run_repeats},
    {"dbg",       CMD_DBG,       FILE_NONE,   1, 0, cmd_dbg},
    {"graph",     CMD_GRAPH,     FILE_NONE,   0, 0, run_graph},
    {"unitigs",   CMD_UNITIGS,   FILE_NONE,   0, 0, run_graph},
    {"bidbg",     CMD_BIDBG,     FILE_NONE,   1, 0, cmd_bidbg},
};

/* one row per option and meaning: the commands that take it (bit c: command c; MAPS: every command whose row says maps; PAIR:
 * any other command answers "only with map"), its kind, where the value goes in struct query_args (at) and which int
 * becomes 1 beside it (mark, 0: none).  FLAG sets an int, BITS ors lo into a u32, U32 and U64 (NUM: by the member's width)
 * take a number in [lo, hi] or print err, STR keeps the argument; FLAG and BITS take no value.  fn, where a row has one,
 * stands in for take(). */
enum kind { FLAG, BITS, U32, U64, STR };
struct option {
    const char *name; uint32_t cmds; enum kind kind; size_t at, mark; uint64_t lo, hi; const char *err;
    int (*fn)(struct query_args *, const struct option *, const char *);
};

static int take(struct query_args *A, const struct option *o, const char *v) {
    void *p = (char *)A + o->at;
    uint64_t x = 0;
    if ((o->kind == U32 || o->kind == U64) && (parse_u64(v, &x) || x < o->lo || x > o->hi)) { fprintf(stderr, "%s: %s\n", o->name, o->err); return 1; }
    if (o->kind == FLAG) *(int *)p = 1;
    else if (o->kind == BITS) *(uint32_t *)p |= (uint32_t)o->lo;
    else if (o->kind == U32) *(uint32_t *)p = (uint32_t)x;
    else if (o->kind == U64) *(uint64_t *)p = x;
    else *(const char **)p = v;
    if (o->mark) *(int *)((char *)A + o->mark) = 1;
    return 0;
}

static int opt_threads(struct query_args *A, const struct option *o, const char *v) {
    if (take(A, o, v)) return 1;
    if (A->threads > 256) A->threads = 256;
    return 0;
}

static int opt_sa_sample(struct query_args *A, const struct option *o, const char *v) {
    if (take(A, o, v)) return 1;
    if (A->sa_sample & (A->sa_sample - 1)) { fprintf(stderr, "%s: %s\n", o->name, o->err); return 1; }
    return 0;
}

static int opt_insert(struct query_args *A, const struct option *o, const char *v) {
    uint64_t lo = 0, hi = 0;
    char buf[48];
    const char *comma = strchr(v, ',');
    if (!comma || (size_t)(comma - v) >= sizeof buf) { fprintf(stderr, "--insert: LO,HI, two template lengths\n"); return 1; }
    memcpy(buf, v, (size_t)(comma - v)); buf[comma - v] = 0;
    if (parse_u64(buf, &lo) || parse_u64(comma + 1, &hi) || lo > hi || hi < 1 || hi > DEBWT_FM_INSERT_MAX) {
        fprintf(stderr, "--insert: LO,HI with LO <= HI, HI in 1..%u\n", DEBWT_FM_INSERT_MAX);
        return 1;
    }
    A->po.ins_lo = (uint32_t)lo; A->po.ins_hi = (uint32_t)hi; A->insert_given = 1;
    return 0;
}

static int opt_min_count(struct query_args *A, const struct option *o, const char *v) {
    A->auto_count = !strcmp(v, "auto");
    return A->auto_count ? 0 : take(A, o, v);
}

static int opt_forward(struct query_args *A, const struct option *o, const char *v) {
    A->ko.flags &= ~DEBWT_FM_BOTH_STRANDS;
    return 0;
}

static int opt_kind(struct query_args *A, const struct option *o, const char *v) {          /* --supermaximal, --intervals */
    if (A->kind_given) { fprintf(stderr, "--supermaximal, --intervals: one of the two\n"); return 1; }
    A->kind = (uint32_t)o->lo; A->kind_given = 1;
    return 0;
}

#define AT(member) offsetof(struct query_args, member)
#define NUM(member) (sizeof ((struct query_args *)0)->member == 8 ? U64 : U32), AT(member)   /* as wide as the member is */
#define C(c) (1u << CMD_##c)
#define MAPS (1u << 31)
#define PAIR (1u << 30)
#define PILES (C(PILEUP) | C(CONSENSUS))
#define GRAPHS (C(GRAPH) | C(UNITIGS))
_Static_assert(DEBWT_FM_CORRECT_MAX_ROUNDS == 16 && DEBWT_FM_ESA_MAX_K == 4096, "the texts of --rounds and --profile name them");
static const struct option options[] = {
    {"-i", ~PAIR, STR, AT(out)},
    {"--device", ~PAIR, NUM(device), 0, 0, 255, "a GPU ordinal"},
    {"-t", C(INDEX) | MAPS, NUM(threads), 0, 1, UINT64_MAX, "thread number must be a positive integer", opt_threads},
    {"--iupac", C(INDEX) | MAPS, NUM(seed), AT(iupac), 0, UINT64_MAX, "a seed"},
    {"--sa", C(INDEX), NUM(sa_sample), 0, 1, 1024, "a power of two in 1..1024", opt_sa_sample},
    {"--sa", C(LCP), STR, AT(sa_file)},
    {"--both-strands", C(COUNT) | C(LOCATE) | C(MEMS) | C(OVERLAPS) | C(KMERS), BITS, AT(flags), AT(search), DEBWT_FM_BOTH_STRANDS},
    {"--both-strands", GRAPHS, FLAG, AT(both)},
    {"--best", C(COUNT) | C(LOCATE), BITS, AT(flags), AT(search), DEBWT_FM_BEST_ONLY},
    {"--mismatches", C(COUNT) | C(LOCATE), NUM(mismatches), AT(search), 0, 4, "a count in 0..4"},
    {"--records", C(COUNT), FLAG, AT(count_records)},
    {"--max-hits", C(LOCATE) | C(MEMS), NUM(max_hits), 0, 0, UINT64_MAX, "a count"},
    {"--min-len", C(MEMS), NUM(mem_len), 0, 1, UINT32_MAX, "a length of at least 1"},
    {"--min-len", MAPS, NUM(mo.min_len), 0, 1, UINT32_MAX, "a length of at least 1"},
    {"--min-len", C(REPEATS) | C(MUMS), NUM(min_len), 0, 1, UINT32_MAX, "a length of at least 1"},
    {"--ref", MAPS, STR, AT(ref)},
    {"--band", MAPS, NUM(mo.band), 0, 0, 63, "a half-width in 0..63"},
    {"--max-occ", MAPS, NUM(mo.max_occ), 0, 1, UINT32_MAX, "a count of at least 1"},
    {"--max-occ", C(REPEATS), NUM(max_occ), 0, 2, UINT64_MAX, "a number of occurrences of at least 2"},
    {"--min-score", MAPS, NUM(mo.min_score), 0, 0, 0x7FFFFFFF, "a score of at least 0"},
    {"--chain", MAPS, FLAG, AT(chain)},
    {"--max-gap", MAPS, NUM(co.max_gap), AT(gap_given), 0, UINT32_MAX, "a length of at least 0"},
    {"--mate", MAPS | PAIR, STR, AT(mate)},
    {"--insert", MAPS | PAIR, STR, 0, 0, 0, 0, NULL, opt_insert},
    {"--no-rescue", MAPS | PAIR, FLAG, AT(no_rescue)},
    {"--min-mapq", PILES, NUM(min_mapq), 0, 0, 60, "a quality in 0..60"},
    {"--region", PILES, STR, AT(region)},
    {"--window", PILES, NUM(window), 0, 1, 1ull << 32, "positions per table, 1..2^32"},
    {"--min-depth", PILES, NUM(call.min_depth), 0, 0, UINT32_MAX, "a depth of at least 0"},
    {"--min-permille", PILES, NUM(call.min_permille), 0, 0, 1000, "a share in 0..1000"},
    {"--variants", C(CONSENSUS), STR, AT(variants)},
    {"--min-overlap", C(OVERLAPS) | GRAPHS, NUM(min_overlap), 0, 1, UINT32_MAX, "a length of at least 1"},
    {"--longest", C(OVERLAPS), BITS, AT(flags), 0, DEBWT_FM_OVERLAP_LONGEST},
    {"--no-self", C(OVERLAPS), FLAG, AT(no_self)},
    {"--max-mismatches", C(OVERLAPS), NUM(ovl_k), AT(ovl_mm), 0, 4, "a count in 0..4"},
    {"--max-error-permille", C(OVERLAPS), NUM(ovl_permille), AT(permille_given), 0, 1000, "a rate in 0..1000"},
    {"--all", C(EXTRACT), FLAG, AT(all)},
    {"-k", C(KMERS) | C(CORRECT), NUM(ko.k), AT(k_given), 1, UINT32_MAX, "a k-mer length of at least 1"},
    {"-k", C(SPECTRUM), NUM(ko.k), AT(k_given), 1, 32, "a k-mer length in 1..32"},
    {"-k", C(DBG) | C(BIDBG), NUM(ko.k), AT(k_given), 1, UINT32_MAX - 1, "a k-mer length in 1..2^32-2"},
    {"--min-count", C(CORRECT), NUM(ko.min_count), 0, 1, UINT32_MAX, "a count of at least 1", opt_min_count},
    {"--rounds", C(CORRECT), NUM(ko.max_rounds), 0, 1, DEBWT_FM_CORRECT_MAX_ROUNDS, "a number in 1..16"},
    {"--forward", C(CORRECT) | C(SPECTRUM), FLAG, 0, 0, 0, 0, NULL, opt_forward},
    {"--report", C(CORRECT), STR, AT(report)},
    {"--bins", C(SPECTRUM), NUM(bins), 0, 2, 4096, "a number of bins in 2..4096"},
    {"--list", C(SPECTRUM), STR, AT(list)},
    {"--at-least", C(SPECTRUM), NUM(at_least), AT(filter_given), 1, UINT32_MAX, "a multiplicity of at least 1"},
    {"--at-most", C(SPECTRUM), NUM(at_most), AT(filter_given), 1, UINT32_MAX, "a multiplicity of at least 1"},
    {"--max-lcp", C(LCP) | C(REPEATS), NUM(max_lcp), 0, 1, UINT32_MAX, "a cap of at least 1"},
    {"--lcp", C(LCP), STR, AT(lcp_file)},
    {"--da", C(LCP), STR, AT(da_file)},
    {"--profile", C(LCP), NUM(profile_k), 0, 1, DEBWT_FM_ESA_MAX_K, "a length in 1..4096"},
    {"--min-occ", C(REPEATS), NUM(min_occ), 0, 2, UINT64_MAX, "a number of occurrences of at least 2"},
    {"--supermaximal", C(REPEATS), FLAG, 0, 0, DEBWT_FM_REPEAT_SUPERMAXIMAL, 0, NULL, opt_kind},
    {"--intervals", C(REPEATS), FLAG, 0, 0, DEBWT_FM_REPEAT_INTERVALS, 0, NULL, opt_kind},
    {"--seq", C(REPEATS) | C(MUMS), FLAG, AT(seq)},
    {"--occurrences", C(REPEATS), FLAG, AT(occurrences)},
    {"--min-records", C(REPEATS) | C(MUMS), NUM(min_records), AT(by_record), 1, UINT64_MAX, "a number of records of at least 1"},
    {"--max-records", C(REPEATS), NUM(max_records), AT(by_record), 1, UINT64_MAX, "a number of records of at least 1"},
    {"--unique", C(REPEATS), FLAG, AT(unique), AT(by_record)},
    {"--fasta", C(DBG) | C(BIDBG), FLAG, AT(fasta)},
    {"--all-edges", C(GRAPH), FLAG, AT(all_edges)},
    {"--states", GRAPHS, STR, AT(states)},
    {"--clean", GRAPHS, FLAG, AT(clean)},
    {"--max-tip", GRAPHS, NUM(cl.max_tip), AT(clean), 0, UINT32_MAX, "a number of reads of at least 0"},
    {"--max-bubble", GRAPHS, NUM(cl.max_bubble), AT(clean), 0, UINT32_MAX, "a number of reads of at least 0"},
    {"--clean-rounds", GRAPHS, NUM(cl.max_rounds), AT(clean), 1, UINT32_MAX, "a number of at least 1"},
};

/* the row of option `name` for a command of mask `cmds`, or NULL */
static const struct option *find_option(const char *name, uint32_t cmds) {
    for (size_t j = 0; j < sizeof options / sizeof *options; j++)
        if ((options[j].cmds & cmds) && !strcmp(options[j].name, name)) return options + j;
    return NULL;
}

/* the defaults of every command, before its options are read */
static void set_defaults(struct query_args *A, const struct command *c) {
    memset(A, 0, sizeof *A);
    A->cmd = c->cmd; A->name = c->name;
    A->threads = 8; A->sa_sample = 32; A->mem_len = 19; A->min_overlap = 20; A->window = 1ull << 26; A->min_mapq = 20;
    A->bins = 256; A->at_least = 1; A->at_most = UINT32_MAX; A->min_len = 20; A->kind = DEBWT_FM_REPEAT_MAXIMAL; A->min_occ = 2;
    debwt_fm_map_defaults(&A->mo); debwt_fm_chain_defaults(&A->co); debwt_fm_pair_defaults(&A->po);
    debwt_fm_pile_defaults(&A->call); debwt_fm_correct_defaults(&A->ko); debwt_fm_clean_defaults(&A->cl);
}

/* reads the arguments behind the command into A.  0: done; 1: an option has said what is wrong with it; 2: the usage text does */
static int parse_options(struct query_args *A, const struct command *c, int argc, char **argv) {
    const uint32_t me = 1u << c->cmd | (c->maps ? MAPS : 0);
    for (int i = 2; i < argc; i++) {
        const char *a = argv[i], *v = NULL;
        if (a[0] != '-' || !a[1]) {
            if (A->file) return 2;
            A->file = a;
            continue;
        }
        const struct option *o = find_option(a, me);
        if (!o && find_option(a, PAIR)) { fprintf(stderr, "%s: only with map\n", a); return 1; }
        if (!o || o->kind >= U32) {                       /* a value follows; an option that is none of this command's ends here */
            if (i + 1 >= argc || !o) return 2;
            v = argv[++i];
        }
        if (o->fn ? o->fn(A, o, v) : take(A, o, v)) return 1;
    }
    return 0;
}

int main(int argc, char **argv) {
    const struct command *c = NULL;
    for (size_t j = 0; argc >= 2 && j < sizeof commands / sizeof *commands; j++)
        if (!strcmp(commands[j].name, argv[1])) c = commands + j;
    if (!c) { usage(); return 1; }
    struct query_args A;
    set_defaults(&A, c);
    const int rc = parse_options(&A, c, argc, argv);
    if (rc == 1) return 1;
    const int file_ok = c->file == FILE_NEEDED ? A.file != NULL : c->file == FILE_NONE ? !A.file : !A.all != !A.file;
    if (rc || !A.out || !file_ok) { usage(); return 1; }
    if (c->need_k && !A.k_given) { fprintf(stderr, "%s: -k K is required\n", c->name); usage(); return 1; }
    return c->run(&A);
}
