/*
 * mhx.h -- C ABI of the MI355X-native MinHash sketch + distance engine ("mhx").
 *
 * This library is the in-process replacement for the `mash` child processes that
 * AuriClass spawns.  Every entry point names the reference interface it replaces
 * (paths relative to /root/reference):
 *
 *   mhx_sketch_files  <- `mash sketch [-r -m M] -o OUT -k K -s S files...`
 *                        auriclass/classes.py:576-596 (FASTQ) and :696-713 (FASTA)
 *   mhx_sketch_files_individual <- `mash sketch -i -o OUT -k K -s S files...` (not called by AuriClass: how a reference
 *                        set is made from one multi-FASTA, docs/faq.md "I want to build my own database")
 *   mhx_dist_files    <- `mash dist REF.msh QUERY.msh`      auriclass/classes.py:92-104
 *   mhx_dist_files_multi <- `mash dist REF.msh QUERY.msh [QUERY.msh ...]` (a run of samples, one call)
 *   mhx_triangle_files <- `mash triangle [-E] [-C] [-d D] [-v V] SET.msh [SET.msh ...]` (not called by AuriClass: all
 *                        pairs within a reference set -- duplicates, the matrix a tree starts from, how far the clades are apart)
 *   mhx_search_files  <- no mash command: `mash dist REF.msh QUERY.msh ...` followed by a sort per query, for a reference
 *                        set too large to print in full -- per query sketch the `top` closest references within a
 *                        distance bound, as dist rows (python -m auriclass_amd.search)
 *   mhx_dist_support  <- no mash command, and what AuriClass's QC_multiple_hits reads off one cell of `mash bounds`: a jackknife
 *                        over the sketch hashes -- in how many resampled sketches each of a query's closest references is still
 *                        the best one (buffer level; engine.dist_support)
 *   mhx_search_files_support <- no mash command: the same for sketch files, as further columns of the search's rows, with the
 *                        clades of AuriClass's clade_config.csv (python -m auriclass_amd.search --support R [--clades FILE])
 *   mhx_contain_files <- no mash command, and what `mash screen` answers from the reads: which share of each reference's
 *                        hashes a sample holds, from the two sketch files alone -- a contaminated or mixed sample keeps
 *                        its identity where `mash dist` loses it (python -m auriclass_amd.contain; buffer level: mhx_dist_contain)
 *   mhx_contain_files_winner <- no mash command, `mash screen -w` for two sketch files: every shared hash credited to its best
 *                        reference, so that the members of a clade stop repeating one another's row (python -m
 *                        auriclass_amd.contain -w; buffer level: mhx_dist_contain_winner)
 *   mhx_contain_files_search <- no mash command: mhx_contain_files followed by a sort per query, for a reference set too
 *                        large to print in full -- per query sketch the `top` references it holds the largest share of
 *                        (python -m auriclass_amd.contain -n TOP; buffer level: mhx_dist_contain_search)
 *   mhx_contain_files_within <- no mash command: mhx_contain_files followed by a filter, for a reference set too large for
 *                        the full table -- per query sketch EVERY reference it holds, with no cap, as CSR
 *                        (python -m auriclass_amd.contain --all; buffer level: mhx_dist_contain_within)
 *   mhx_cluster_files <- no mash command: `mash triangle -E -d D` followed by a union-find over its edge list -- which
 *                        references of a set are the same thing within distance D, and one representative of each, as a
 *                        table and as a dereplicated sketch file (python -m auriclass_amd.cluster)
 *   mhx_dist_medoids  <- no mash command: `mash triangle` followed by per-cluster sums on the host -- the member of every
 *                        cluster with the smallest sum of distances to the others (buffer level; engine.dist_medoids, and
 *                        mhx_dist_to: every list against one target)
 *   mhx_cluster_reps_files <- no mash command: the dereplication for every linkage with the medoid as a third kind of
 *                        representative and the distance of every member to its representative as columns
 *                        (python -m auriclass_amd.cluster --rep medoid / --dist)
 *   mhx_dist_mst      <- no mash command: `mash triangle` followed by a sort of all pairs and a union-find -- the single-
 *                        linkage tree of a set, every cut of mhx_dist_cluster at once (buffer level; engine.dist_mst)
 *   mhx_tree_files    <- no mash command: the same for sketch files, as a table of merges or a Newick dendrogram
 *                        (python -m auriclass_amd.tree)
 *   mhx_dist_linkage  <- no mash command: `mash triangle` followed by a hierarchical clustering on the host -- complete and
 *                        average linkage (UPGMA) of a set on the device (buffer level; engine.dist_linkage)
 *   mhx_linkage_files <- no mash command: the same for sketch files, as merges, a Newick dendrogram or the cut at a distance
 *                        (python -m auriclass_amd.tree / auriclass_amd.cluster --linkage complete|average)
 *   mhx_dist_nj       <- no mash command: `mash triangle` followed by a neighbour-joining tool on the host (the mashtree
 *                        workflow) -- the unrooted tree of a set on the device (buffer level; engine.dist_nj)
 *   mhx_nj_files      <- no mash command: the same for sketch files, as a table of joins or an unrooted Newick tree
 *                        (python -m auriclass_amd.tree --nj)
 *   mhx_dist_nj_support <- no mash command: a jackknife over the sketch hashes (as the tools that build Mash trees ship one) --
 *                        in how many trees of resampled sketches each split of the neighbour-joining tree is found
 *                        (buffer level; engine.dist_nj_support; mhx_resample_rows is one replicate of a set)
 *   mhx_nj_files_opts <- no mash command: the same for sketch files, the support as a column or as Newick node labels
 *                        (python -m auriclass_amd.tree --nj --support R)
 *   mhx_bounds        <- `mash bounds -k K -p P`            auriclass/classes.py:305-318
 *   mhx_screen_files  <- `mash screen REF.msh reads...`     (not called by AuriClass: the containment question its
 *                        distance check cannot answer, docs/faq.md entries 3 and 4)
 *   mhx_init          <- `mash -h` dependency probe         auriclass/general.py:198-205
 *
 * The remaining entry points expose the same hot path at buffer granularity (device
 * or host pointers) for the throughput benchmark, the multi-GPU shard/merge step and
 * the batched all-vs-refs distance (BASELINE.json configs 3-5).
 *
 * Conventions: plain C types only; the caller owns every buffer; functions return
 * MHX_OK (0) or a negative MHX_E_* code and leave a message for mhx_last_error().
 * Text outputs use the two-call pattern: pass cap = 0 to learn the size in *need
 * (including the terminating NUL), then call again with a buffer of that size.
 * All compute runs on the GPU selected by mhx_init(); there is no CPU fallback:
 * without a usable HIP device every compute entry point fails with MHX_E_NO_DEVICE.
 *
 * One device, one caller: the engine state (device, stream, staging buffers) is a process-wide
 * singleton, as `mash` was one process per sample (docs/running_analysis.md:47-59 of the reference).
 * mhx_init(d) binds the process to GPU d; a second mhx_init with another device tears the first
 * engine down.  Calls are not thread-safe against each other (only mhx_last_error is thread-local).
 * Several GPUs = several processes, one per GPU (auriclass_amd/multigpu.py; bench.py --gpus N).
 */
#ifndef MHX_H
#define MHX_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MHX_OK 0
#define MHX_E_NO_DEVICE (-1)   /* no HIP device / mhx_init not called                  */
#define MHX_E_ARG (-2)         /* bad argument                                          */
#define MHX_E_IO (-3)          /* file cannot be opened / read / written                */
#define MHX_E_NO_RECORDS (-4)  /* "ERROR: Did not find fasta records in ..." (mash)     */
#define MHX_E_FORMAT (-5)      /* malformed FASTA/FASTQ/.msh                            */
#define MHX_E_HIP (-6)         /* HIP runtime error                                     */
#define MHX_E_CAPACITY (-7)    /* caller buffer too small / device table exhausted      */
#define MHX_E_MISMATCH (-8)    /* sketches with different k / seed (mash refuses too)   */
#define MHX_E_INTERNAL (-9)

/* input stream formats for mhx_sketcher_push_* */
#define MHX_FMT_SEQ 0     /* dense sequence bytes; any non-ACGT byte (e.g. '\n') ends a k-mer run */
#define MHX_FMT_FASTQ4 1  /* strict 4-line FASTQ records, parsed on the device                      */
/* A MHX_FMT_FASTQ4 push trusts its caller that every record is clean in the kseq reader's sense: the device checks
 * only that record lines start with '@' and '+'.  A sequence line holding blanks (bytes <= 0x20 or 0x7F, but for one
 * '\r' before its newline) or beginning with '>', '@' or '+', or a quality line with another count of non-blank bytes
 * than its sequence, is read differently by mash and gives a different sketch.  mhx_sketch_files verifies every
 * record of the files it pushes (a separate pass over the bytes, outside the sketch kernel) and hands a file that
 * fails to the host record parser, whose result or refusal is mash's. */

/* ---- library ---------------------------------------------------------------------- */
int mhx_init(int device);              /* selects the GPU, creates the stream; idempotent */
void mhx_shutdown(void);
const char *mhx_last_error(void);      /* thread-local message of the last failure        */
const char *mhx_version(void);
int mhx_device_name(char *buf, size_t cap);

/* ---- file level: what classes.py calls today through subprocess ---------------------- */

/* `mash sketch`.  reads != 0 => `-r -m min_mult`: all files form ONE reference whose
 * length is the set-size estimate; reads == 0 => one reference per file.  Writes the
 * unpacked Cap'n Proto sketch to out_msh and mash's stderr text (incl. the
 * "Estimated genome size: %g" line in reads mode) to stderr_buf.
 * est_genome_size may be NULL. */
int mhx_sketch_files(const char *const *paths, int n_paths, int k, uint32_t s, int reads,
                     uint32_t min_mult, const char *out_msh, char *stderr_buf, size_t stderr_cap,
                     size_t *stderr_need, double *est_genome_size);

/* `mash sketch -i -k K -s S -o OUT files...`: one reference per RECORD, in file order and then record order -- what a
 * reference set for mhx_dist_files / mhx_screen_files is built from when it ships as one multi-FASTA.  name = the record's
 * header up to the first blank, comment = the rest of the header, length = the record's sequence length, hashes = the
 * min(s, distinct) smallest hashes of the record's own windows.  stderr_buf receives the text of
 * mhx_sketch_files(..., reads = 0, ...), *n_refs_out (may be NULL) the number of references written.
 *   - A record shorter than k is left out (the per-file mode does not count it either).
 *   - A record of at least k bytes without one valid window (all N) is kept, with an empty hash list (the per-file mode
 *     keeps a file of such records too).
 *   - A file from which no record remains fails with MHX_E_NO_RECORDS and mash's message.
 * Plain FASTA is parsed on the device, everything else kseq reads (FASTQ, files that do not start with '>') by the host
 * record parser; gzip and BGZF as everywhere.  Both routes end in mhx_sketch_segments.
 * Not pinned by mash output (none is recorded for -i): the result is the oracle's sketch applied record by record; the
 * two record rules above are ours where Mash's source leaves room.  DESIGN.md section 6. */
int mhx_sketch_files_individual(const char *const *paths, int n_paths, int k, uint32_t s, const char *out_msh,
                                char *stderr_buf, size_t stderr_cap, size_t *stderr_need, uint64_t *n_refs_out);

/* `mash dist REF QUERY` stdout: rows "ref\tquery\tdist\tp\tcommon/denom\n", query-major. */
int mhx_dist_files(const char *ref_msh, const char *qry_msh, char *stdout_buf, size_t cap, size_t *need);

/* `mash dist REF QUERY [QUERY ...]` stdout: the rows of mhx_dist_files(ref, qry[0]), then those of
 * qry[1], ... -- query-major in argument order, every sketch of a query file in the file's order.
 * The reference file is read, parsed, order-checked and staged once per call and the sketches of all
 * query files are compared in one device call (mhx_dist_files is the n_qry == 1 case).  n_qry < 1 or a
 * null entry: MHX_E_ARG.  A query file that cannot be read or parsed, or whose k or hash seed differs from
 * the reference's, fails the whole call as it fails mhx_dist_files.  Query files whose sketch sizes differ
 * from each other are refused with MHX_E_MISMATCH: what mash prints for such a set is not pinned by any
 * recorded output, and a run of samples sketched with one setting never produces one.  The effective
 * sketch size is min(reference, query); more than 2^31 - 1 pairs per call are refused (MHX_E_ARG). */
int mhx_dist_files_multi(const char *ref_msh, const char *const *qry_msh, int n_qry,
                         char *stdout_buf, size_t cap, size_t *need);

/* `mash screen REF.msh reads...` stdout (Mash 2.x, nucleotides, every row printed; -w, -i and -v: mhx_screen_files_opts): one row per reference of the
 * sketch file, in its order, "identity\tshared/n\tmedian\tp\tname\tcomment\n".  All paths form ONE read set (FASTQ or
 * FASTA, plain or gzip / BGZF), read by the ingest of mhx_sketch_files(..., reads = 1, ...): every route, the record check
 * and the hand-over to the host record parser included (mhx_last_fastq_route reports this call's route too).
 *   shared   = hashes of the reference sketch that occur in the read set (n = the sketch's length),
 *   median   = element [shared / 2] of the ascending multiplicities of those hashes (0: none),
 *   identity = mhx_screen_identity(shared, n, k),  p = mhx_screen_p_value(shared, n, set size, k),
 *   set size = the estimated number of distinct k-mers of the read set: the "Estimated genome size" of
 *              mhx_sketch_files(paths, k, s, 1, 1, ...) with the reference file's k and sketch size s; handed back in
 *              *set_size_out (may be NULL).
 * A multiplicity is the number of windows (k bytes A/C/G/T inside one record) with that canonical hash, as the sketcher
 * counts them.  A read set without any valid k-mer is no error here: set size 0, rows "0\t0/n\t0\t1\t...".  A reference file
 * with another hash seed than 42 or another alphabet: MHX_E_MISMATCH.  Not pinned by mash output (none is recorded): the
 * rule is Mash's CommandScreen restated, see DESIGN.md section 6. */
int mhx_screen_files(const char *ref_msh, const char *const *paths, int n_paths, char *stdout_buf, size_t cap, size_t *need,
                     double *set_size_out);

/* mhx_screen_files with `mash screen`'s -w, -i and -v.  opts == NULL, or {sizeof, 0, -1, 1}, is mhx_screen_files byte for
 * byte.
 *   winner != 0:   winner-take-all (-w, see mhx_screener_finish_winner); the genome lengths are the reference file's.
 *   min_identity:  -i.  A row is printed when identity >= min_identity; 0 means identity > 0 only, -1 every row.  Mash's
 *                  default is 0, ours stays -1.
 *   max_p_value:   -v.  A row is printed when p <= max_p_value.
 * Both filters compare the doubles of mhx_screen_identity / mhx_screen_p_value on the host; under -w they see the winner
 * rows.  MHX_E_ARG: struct_size != sizeof(mhx_screen_opts), min_identity > 1 or max_p_value outside [0, 1] (or not a
 * number). */
typedef struct mhx_screen_opts {
    uint32_t struct_size; /* sizeof(mhx_screen_opts) */
    int32_t winner;
    double min_identity;
    double max_p_value;
} mhx_screen_opts;
int mhx_screen_files_opts(const char *ref_msh, const char *const *paths, int n_paths, const mhx_screen_opts *opts, char *stdout_buf,
                          size_t cap, size_t *need, double *set_size_out);

/* `mash triangle [-E] [-C] [-d max_dist] [-v max_p_value] a.msh [b.msh ...]` stdout (Mash 2.x CommandTriangle restated).
 * The references of all files form ONE set, in argument order and then file order; every pair j < i of it is compared by
 * mhx_dist_triangle / mhx_dist_triangle_edges.
 *   matrix (edge == 0): "\t<n>\n", then one line per reference i = 0 .. n - 1: its name (comment != 0: its comment),
 *       "\t<distance>" for j = 0 .. i - 1, "\n".
 *   edge list (edge != 0, or max_dist < 1, or max_p_value < 1, as Mash's -d / -v imply -E): no header; for i ascending and
 *       j < i ascending every pair with distance <= max_dist and p <= max_p_value prints
 *       "name_i\tname_j\tdist\tp\tcommon/denom\n" -- a `mash dist` row with reference i and query j,
 *       p = mhx_p_value(common, length_i, length_j, k, denom).
 * opts == NULL means {sizeof, 0, 0, 1, 1}.  All files must share k, hash seed and sketch size (MHX_E_MISMATCH otherwise);
 * a hash list that is not ascending is MHX_E_FORMAT.  MHX_E_ARG: struct_size != sizeof(mhx_triangle_opts), a max_dist or
 * max_p_value that is not a number, more than 65 536 references.
 * Not pinned by mash output (none is recorded for `triangle`): like the screen, the mode is pinned by its restated rule,
 * and its pairs by the mash-pinned distance path (the rows equal those mhx_dist_files prints for the same pairs).
 * DESIGN.md section 6. */
typedef struct mhx_triangle_opts {
    uint32_t struct_size; /* sizeof(mhx_triangle_opts) */
    int32_t edge;
    int32_t comment;
    double max_dist;
    double max_p_value;
} mhx_triangle_opts;
int mhx_triangle_files(const char *const *msh_paths, int n_paths, const mhx_triangle_opts *opts, char *stdout_buf, size_t cap,
                       size_t *need);

/* `mash bounds -k K -p P` stdout. */
int mhx_bounds(int k, double p, char *buf, size_t cap, size_t *need);

/* FASTA base count (replaces pyfastx.Fasta(f).size, classes.py:746-751). */
int mhx_fasta_total_bases(const char *path, uint64_t *total);
/* format sniffing (replaces pyfastx probes, general.py:68-115): 1 yes, 0 no, <0 error */
int mhx_sniff_fastq(const char *path);
int mhx_sniff_fasta(const char *path);
/* the end of a 4-line FASTQ stream (its last bytes, up to 64 KiB are enough): 1 when the last record is complete in kseq's
 * sense, 0 when it has its '+' line but no quality string, one with another count of non-blank bytes than its sequence
 * (kseq_read: -2; such a file is refused by mhx_sketch_files), or a sequence line with a blank inside; callers that push byte ranges of a file themselves ask here for its tail */
int mhx_fastq_tail_complete(const void *tail, size_t n);
/* which parser the last mhx_sketch_files call with reads != 0 took: 0 none (it failed early),
 * MHX_ROUTE_DEVICE_STREAMED (device FASTQ parser, streamed ingest), MHX_ROUTE_DEVICE_WHOLE (device FASTQ parser,
 * whole files), MHX_ROUTE_RECORD_PARSER (host record parser for at least one file) */
#define MHX_ROUTE_DEVICE_STREAMED 1
#define MHX_ROUTE_DEVICE_WHOLE 2
#define MHX_ROUTE_RECORD_PARSER 3
int mhx_last_fastq_route(void);

/* ---- buffer level: the hot path itself ------------------------------------------------ */
typedef struct mhx_sketcher mhx_sketcher;

/* expected_bytes: upper bound of the bytes that will be pushed (sizes the device
 * candidate table and the initial admission threshold); 0 = unknown/small. */
int mhx_sketcher_create(int k, uint32_t s, uint32_t min_mult, uint64_t expected_bytes, mhx_sketcher **out);
/* Same with budget_scale times the candidate table and admission budget: what a caller asks for after
 * finish() has reported MHX_E_CAPACITY (inputs whose solid k-mers are fewer than s when min_mult > 1;
 * the file-level call retries with 16, 256, ... by itself). */
int mhx_sketcher_create_scaled(int k, uint32_t s, uint32_t min_mult, uint64_t expected_bytes, uint32_t budget_scale,
                               mhx_sketcher **out);
void mhx_sketcher_destroy(mhx_sketcher *sk);
int mhx_sketcher_reset(mhx_sketcher *sk);

/* Feed one record-aligned span.  The device pointer must be readable up to the next
 * 16-byte boundary past n (true for any hipMalloc/torch allocation).  Asynchronous on
 * the engine's stream; the buffer must stay valid AND unchanged until mhx_sketcher_finish() or
 * mhx_sketcher_sync() has returned -- a synchronisation of the stream alone is not enough: FASTQ spans
 * whose reads are longer than ~2.7 kb are read a second time by a pass that those two calls start. */
int mhx_sketcher_push_device(mhx_sketcher *sk, const void *d_bytes, uint64_t n, int fmt);
int mhx_sketcher_push_host(mhx_sketcher *sk, const void *h_bytes, uint64_t n, int fmt);
int mhx_sketcher_sync(mhx_sketcher *sk);

/* Final sketch: the s smallest distinct hashes with multiplicity >= min_mult, ascending.
 * hashes/counts must hold s entries (counts may be NULL). */
int mhx_sketcher_finish(mhx_sketcher *sk, uint64_t *hashes, uint32_t *counts, uint32_t *n_out);

/* stats of the pushes so far: [0] k-mers hashed, [1] table inserts, [2] lines seen (FASTQ4),
 * [3] device flags, [4] occupied table slots, [5] hash-kernel ms (profiling on), [6] launches,
 * [7] threshold */
int mhx_sketcher_stats(mhx_sketcher *sk, uint64_t *stats8);
/* FASTQ4 pushes so far: records whose sequence line holds >= k bytes -- the sequences `mash sketch`
 * counts (it skips shorter ones) and reports as "[N seqs]" in the .msh comment */
int mhx_sketcher_record_count(mhx_sketcher *sk, uint64_t *records);
int mhx_sketcher_debug_stamps(mhx_sketcher *sk, uint64_t *out8); /* per-phase cycle sums of a -DMHX_STAMPS diagnostic build */
int mhx_set_profiling(int on);   /* time hash-kernel launches with HIP events on the engine stream */
void *mhx_stream(void);          /* the engine's hipStream_t */

/* Multi-GPU: a shard's partial result = every (hash, count) it saw with hash <= limit
 * (no multiplicity filter).  export_threshold() returns the shard's own admission
 * threshold; ranks exchange the minimum, export with it, all-gather the slabs and merge. */
int mhx_sketcher_threshold(mhx_sketcher *sk, uint64_t *threshold);
int mhx_sketcher_export(mhx_sketcher *sk, uint64_t limit, uint64_t *hashes, uint32_t *counts,
                        uint32_t cap, uint32_t *n_out);
/* Same partial result, left on the device as one slab of int64 words ready for an all-gather:
 * [0] n (entries found; only min(n, cap) are stored), [1] the shard's threshold, [2] device flags,
 * [3, 3+cap) hashes, then cap/2 words holding the u32 counts; every entry <= the threshold, unsorted,
 * no multiplicity filter.  cap must be even.  The hash value 2^64-1 is not representable here: callers
 * fall back to mhx_sketcher_export when a threshold of 2^64-1 comes back. */
int mhx_sketcher_export_slab(mhx_sketcher *sk, void *d_slab, uint32_t cap);
/* The sharded path as the ranks run it (auriclass_amd/multigpu.py; SURVEY.md 8(e): sizes first, slabs sized from the
 * data, merge where the data is).  Replaces nothing in the reference by itself: it is how `mash sketch -r -m M` over ONE
 * sample (auriclass/classes.py:576-596) is spread over the GPUs of a node.
 *   1. mhx_sketcher_export_begin: every (hash, count) of this shard with hash <= its threshold T_r (no multiplicity
 *      filter) is compacted into a device buffer of the sketcher; header8 receives [0] n_r, [1] T_r, [2] device flags |
 *      MHX_SLAB_* bits, [3] occurrences of the hash value 2^64-1, [4] occupied table slots, [5..7] 0.  Ranks all-gather
 *      these 64 bytes.
 *   2. mhx_sketcher_export_pack: the entries as one slab of 8-byte words, hashes[cap_entries] then the u32 counts
 *      (cap_entries even, >= n_r; normally max_r n_r rounded up), written to dst -- device memory (RCCL send buffer) or
 *      host memory (gloo).  Entries beyond n_r are unspecified.  Ranks all-gather the slabs.
 *   3. mhx_sketcher_merge_slabs: slabs = the n_ranks gathered slabs back to back (slabs_on_device != 0: device
 *      memory), headers = the n_ranks gathered headers (8 words each).  The other ranks' entries <= T_min = min_r T_r
 *      are added to this rank's candidate table on the device and the union's sketch is extracted: the first s hashes
 *      with summed multiplicity >= min_mult.  MHX_E_CAPACITY if fewer than s qualify below a lowered T_min (every rank
 *      gets the same verdict from the same gathered data and sketches its shard again with a larger budget_scale).
 *      The sketcher's table now holds other shards' entries: mhx_sketcher_reset() before it is used again. */
int mhx_sketcher_export_begin(mhx_sketcher *sk, uint64_t *header8);
int mhx_sketcher_export_pack(mhx_sketcher *sk, void *dst, uint64_t cap_entries);
int mhx_sketcher_merge_slabs(mhx_sketcher *sk, const void *slabs, int slabs_on_device, uint32_t n_ranks,
                             uint64_t cap_entries, const uint64_t *headers, uint32_t own_rank, uint64_t *hashes,
                             uint32_t *counts, uint32_t *n_out);
/* The same exchange in ONE collective, for slabs that live on the device (RCCL): the header rides in front of the slab,
 * [header8 | hashes[cap_entries] | counts u32[cap_entries]] = 8 + cap_entries + cap_entries / 2 words.
 * mhx_sketcher_export_into compacts the shard's partial result straight into the caller's send buffer (header8 as for
 * export_begin; entries beyond cap_entries are counted in [0] but not stored).  After the all-gather,
 * mhx_sketcher_merge_gathered reads the headers back, and either merges (as mhx_sketcher_merge_slabs) or, when some shard
 * holds more entries than the slabs have room for, returns MHX_E_CAPACITY with *need_cap = the largest n_r: every rank
 * gets the same answer from the same gathered headers and repeats both calls with a larger cap_entries.  *need_cap == 0
 * with MHX_E_CAPACITY is the exactness rule's verdict (re-sketch with a larger budget_scale). */
int mhx_sketcher_export_into(mhx_sketcher *sk, void *d_slab, uint64_t cap_entries, uint64_t *header8);
int mhx_sketcher_merge_gathered(mhx_sketcher *sk, const void *d_slabs, uint32_t n_ranks, uint64_t cap_entries,
                                uint32_t own_rank, uint64_t *hashes, uint32_t *counts, uint32_t *n_out,
                                uint64_t *need_cap);
/* The last merge on this sketcher (read-only): info8[0] the path that produced the answer -- MHX_MERGE_BINNED (value bins
 * merged in LDS), MHX_MERGE_TABLE (the other ranks' entries added to the candidate table) or MHX_MERGE_HOST (the host
 * merge on the gathered data); 0 before the first merge, and when the last merge call was rejected before any path ran (the info is
 * cleared at the entry of every merge call; mhx_sketcher_reset() keeps it) --, [1] 1 if the binned
 * merge ran, and then [2] the flags word it returned (1 a bin's region overflowed, 2 a bin's table guard, 4 too many
 * entries qualify in one bin, 8 a summed count passed 2^32-1; any of them sends the call on to the table path),
 * [3] its bins, [4] entries per bin region, [5] slots of a bin's table; [6..7] 0. */
#define MHX_MERGE_BINNED 1
#define MHX_MERGE_TABLE 2
#define MHX_MERGE_HOST 3
int mhx_sketcher_merge_info(mhx_sketcher *sk, uint64_t *info8);
int mhx_merge_partials(const uint64_t *hashes, const uint32_t *counts, uint64_t n, uint32_t s,
                       uint32_t min_mult, uint64_t *out_hashes, uint32_t *out_counts, uint32_t *n_out);
/* bits a shard adds to word [2] of its slab besides the device flags (diagnostics of the m > 1 phase) */
#define MHX_SLAB_BOUNDED 0x100      /* a host-imposed cap has limited the shard's threshold at least once  */
#define MHX_SLAB_ESTABLISHED 0x200  /* the threshold has since been lowered from solid (count >= m) hashes */
/* The merge step of the sharded path together with its exactness rule: hashes/counts are the shards'
 * exports back to back (shard r contributes shard_n[r] entries, all <= shard_threshold[r]).  Entries above
 * T_min = min_r shard_threshold[r] are dropped (only below it is every shard's list complete), counts of equal
 * hashes are summed, count >= min_mult kept, first s returned.  If fewer than s qualify although some shard
 * has rejected hashes (T_min below the largest hash value of this k), the union cannot be decided from these
 * partials: MHX_E_CAPACITY -- every rank sketches its shard again with a larger budget_scale
 * (mhx_sketcher_create_scaled) and the exchange is repeated; a short sketch is never returned in that case.
 * SURVEY.md 8(e); the m = 3 default of /root/reference/auriclass/args.py:128-134 is what makes this matter. */
int mhx_merge_shard_partials(const uint64_t *hashes, const uint32_t *counts, const uint64_t *shard_n,
                             const uint64_t *shard_threshold, uint32_t n_shards, int k, uint32_t s,
                             uint32_t min_mult, uint64_t *out_hashes, uint32_t *out_counts, uint32_t *n_out);

/* Batched all-vs-refs `mash dist` arithmetic on the device: q and r are row-major
 * [n][stride] ascending unique hash lists with q_len/r_len valid entries each.
 * Outputs are [nq][nr] row-major (query-major like mash): common, denom, distance.
 * device_ptrs != 0 => q, r, q_len, r_len, common, denom, dist are device pointers. */
int mhx_dist_batch(const uint64_t *q, const uint32_t *q_len, uint32_t nq, const uint64_t *r,
                   const uint32_t *r_len, uint32_t nr, uint32_t stride, int k, uint32_t s,
                   uint32_t *common, uint32_t *denom, double *dist, int device_ptrs);
double mhx_last_dist_kernel_ms(void);
/* diagnostics of the last mhx_dist_batch / mhx_dist_files / mhx_dist_triangle* / mhx_dist_cluster / mhx_dist_search / mhx_dist_within call: -1 = the generic pair kernel did all the work (tiny batch),
 * else the number of (query batch, reference slice) blocks the all-vs-refs fast path gave up to it (0 for uniform hashes) */
int mhx_last_dist_fallback_blocks(void);
/* value ranges every (query batch, reference slice) block of that call was cut into: 1024 x W, W = the smallest power of two
 * with longest list / (1024 W) <= 64 (1024 for lists of up to 65 536 hashes, 16 384 for 1 000 000; the longest list is taken
 * from q_len / r_len, from `stride` when they are device pointers).  0 = the generic pair kernel did all the work: a tiny
 * batch, lists of more than 2^20 hashes, or every block gave up */
int mhx_last_dist_ranges(void);

/* All pairs j < i of ONE set (`mash triangle` at buffer level): rows / len as mhx_dist_batch takes a list matrix,
 * [n][stride] ascending unique hashes with len[i] valid entries.  Outputs are packed, [n (n - 1) / 2], pair (i, j) at
 * i (i - 1) / 2 + j: the lower triangle row by row, Mash's print order.  dist may be NULL.  n <= 1 is MHX_OK with nothing
 * written; n > 65 536 (more than 2^31 - 1 pairs) is MHX_E_ARG; k, s, stride and len[i] > stride are checked as in
 * mhx_dist_batch.  device_ptrs != 0 => rows, len, common, denom, dist are device pointers and dist is the device's log;
 * with host pointers the distances are libm doubles computed on the host, as in mhx_dist_batch.
 * The set is split into value ranges once per call; slices of 32 lists are the references of a block, the lists behind
 * a slice's first its queries.  The number of ranges follows the longest list (len, or stride
 * when the lengths are on the device): the smallest power of two R with longest <= 16 R, between 16 and 16 384 -- 64 at
 * s = 1000; MHX_TRI_GEOMETRY=dist takes mhx_dist_batch's geometry instead, MHX_TRI_QBATCH bounds the queries of a block.
 * mhx_last_dist_kernel_ms, mhx_last_dist_fallback_blocks and mhx_last_dist_ranges report this call too. */
int mhx_dist_triangle(const uint64_t *rows, const uint32_t *len, uint32_t n, uint32_t stride, int k, uint32_t s,
                      uint32_t *common, uint32_t *denom, double *dist, int device_ptrs);
/* The pairs with distance <= max_dist only, as an edge list (i, j, common, denom, dist) of at most cap entries; nothing of
 * size n^2 is materialised.  *n_out (a HOST pointer in both forms) receives the number of edges; when cap is too small
 * the call returns MHX_E_CAPACITY, *n_out is the number needed and the buffers hold nothing of use.  dist may be NULL.
 * Host pointers: the device prefilters by the Jaccard index of max_dist (lowered by 2^-30 relative), the host applies
 * the exact rule -- the libm distance, the double that is printed, <= max_dist -- and sorts: ascending by (i, j).
 * device_ptrs != 0: edge_i, edge_j, common, denom, dist are device buffers and the list STAYS on the device: prefiltered
 * only (a pair within 1e-9 relative of the bound in the Jaccard index may be in it although its distance rounds above
 * max_dist) and in the order of arrival, which changes from run to run; dist is the device's log. */
int mhx_dist_triangle_edges(const uint64_t *rows, const uint32_t *len, uint32_t n, uint32_t stride, int k, uint32_t s,
                            double max_dist, uint32_t *edge_i, uint32_t *edge_j, uint32_t *common, uint32_t *denom,
                            double *dist, uint64_t cap, uint64_t *n_out, int device_ptrs);

/* Single-linkage clustering of ONE set (dereplication at buffer level): rows / len / n / stride / k / s as
 * mhx_dist_triangle takes them, with its checks (n > 65 536, k, s, stride, len[i] > stride, null pointers: MHX_E_ARG; a
 * max_dist that is not a number too), before anything is launched.
 * Edge: lists i and j are neighbours iff the distance mhx_dist_triangle computes for the pair on the host (libm) is
 * <= max_dist -- the rule of mhx_dist_triangle_edges' host form.  Two empty lists have distance 0: neighbours for any
 * max_dist >= 0; max_dist < 0 gives no edge, max_dist >= 1 makes every pair one.
 * Outputs: label[n], label[i] = the LOWEST index in the connected component of i, so the result does not depend on the
 * order in which the device meets the pairs; degree[n] (may be NULL) the neighbours of i; *n_clusters the lists with
 * label[i] == i; *n_edges the edges.  n_clusters and n_edges are HOST pointers in both forms.  n == 0: MHX_OK, 0 clusters;
 * n == 1: label[0] = 0, 1 cluster.
 * device_ptrs != 0 => rows, len, label and degree are device pointers, and the result is EXACT in this form as well --
 * unlike the device form of mhx_dist_triangle_edges, whose list is prefiltered only: the host turns max_dist into a table
 * cmin[0 .. s] with libm once per call (cmin[d] = the smallest common with distance(common, d) <= max_dist) and the
 * device keeps a pair iff common >= cmin[denom], in integers.  Two calls on the same input give identical outputs.
 * The triangle's blocks feed a lock-free union-find on the device: no edge list and nothing of
 * size n^2 exists anywhere; the workspace is the triangle's plus 4 (s + 1) bytes.  Geometry, MHX_TRI_GEOMETRY and
 * MHX_TRI_QBATCH are the triangle's; mhx_last_dist_kernel_ms, mhx_last_dist_fallback_blocks and mhx_last_dist_ranges
 * report this call too.  Not lifted here: the limit of 65 536 lists.  Complete and average linkage: mhx_dist_linkage below. */
int mhx_dist_cluster(const uint64_t *rows, const uint32_t *len, uint32_t n, uint32_t stride, int k, uint32_t s, double max_dist,
                     uint32_t *label, uint32_t *degree, uint32_t *n_clusters, uint64_t *n_edges, int device_ptrs);
/* The same at file level: the references of all files form one set, read and checked as mhx_triangle_files does (k / seed /
 * sketch-size mismatches MHX_E_MISMATCH, damaged files, at most 65 536 references).  Clusters are numbered from 1 in the
 * order of their lowest member, members in index order; one row per reference, names (comments when `comment` is set):
 *     cluster\tsize\trepresentative\tmember\tdegree\n
 * The representative of a cluster is its lowest index (rep = 0, "first") or its member of greatest genome length, ties to
 * the lower index (rep = 1, "longest").  out_msh (may be NULL): the representatives in cluster order, with their names,
 * comments, lengths and hash lists unchanged, written as mhx_msh_write writes them -- a set that mhx_search_files,
 * mhx_dist_files and mhx_screen_files read; when a reference of the set carries multiplicity counts, which that file
 * cannot store, out_msh is refused with MHX_E_ARG (nothing is dropped silently).  opts == NULL means {sizeof, 0, 0, 1.0}.
 * MHX_E_ARG: struct_size != sizeof(mhx_cluster_opts), rep outside 0 .. 1, a max_dist that is not a number.  Not pinned by
 * mash output (mash has no such command): pinned by the restated rule (tests/cluster_rule.py), its pairs by the
 * mash-pinned distance path.  No p-value filter; the medoid as representative and the distance-to-representative columns
 * are mhx_cluster_reps_files' below. */
typedef struct mhx_cluster_opts {
    uint32_t struct_size; /* sizeof(mhx_cluster_opts) */
    int32_t comment;      /* non-zero: print comments in place of names */
    int32_t rep;          /* 0 first, 1 longest */
    double max_dist;      /* neighbours: distance <= max_dist */
} mhx_cluster_opts;
int mhx_cluster_files(const char *const *msh_paths, int n_paths, const mhx_cluster_opts *opts, const char *out_msh, char *stdout_buf,
                      size_t cap, size_t *need);

/* MEDOIDS of a partition of ONE set: rows / len / n / stride / k / s as mhx_dist_triangle takes them, with its checks, and
 * s >= 2^20 -> MHX_E_ARG as for mhx_dist_linkage.  label[n] is a partition as mhx_dist_cluster, mhx_mst_labels and
 * mhx_linkage_labels return one -- label[i] the lowest index of i's cluster -- and ANY array with label[i] <= i and
 * label[label[i]] == label[i] for all i is taken; another one is MHX_E_ARG.
 * sum[i] (may be NULL) is the sum of mhx_linkage_fixed_distance(common, denom, k) (units of 2^-32) over the other members j
 * of i's cluster, (common, denom) by the pair rule of the mash-pinned distance path; medoid[i] is the member of i's cluster
 * with the smallest (sum, index) -- ties go to the lower index; a list on its own is its medoid with sum 0.  common[n] /
 * denom[n] (both or neither, else MHX_E_ARG): the pair (i, medoid[i]) as mhx_dist_to gives it.
 * device_ptrs != 0 => rows, len, label, medoid, sum, common and denom are device pointers.  In both forms label is
 * validated on the HOST before anything is launched (the device form copies its 4 n bytes back first), so no kernel
 * indexes with an unchecked value.  Every result is an exact integer: the sums are 64-bit integer atomics, the pick a 64-bit
 * minimum over sum << 16 | index; two calls give identical outputs and the two forms agree bit for bit.
 * Only the blocks of the triangle's schedule that hold a pair of one cluster are run (an exact test on the host,
 * 32 binary searches per block); with all singletons nothing of the triangle is launched.  mhx_last_medoid_blocks: blocks the last call ran
 * << 32 | blocks of the schedule.  Device memory: 16 n bytes on top of the triangle's workspace, nothing of size n^2.
 * n == 0: MHX_OK; n == 1: medoid 0, sum 0 and the pair (0, 0), no triangle pass.  Geometry, MHX_TRI_GEOMETRY,
 * MHX_TRI_QBATCH and MHX_DIST_GENERIC are the triangle's.  Not built: more than 65 536 lists,
 * medoids of the neighbour-joining tree, a per-cluster radius (it follows from the pair columns on the host). */
int mhx_dist_medoids(const uint64_t *rows, const uint32_t *len, uint32_t n, uint32_t stride, int k, uint32_t s, const uint32_t *label,
                     uint32_t *medoid, uint64_t *sum, uint32_t *common, uint32_t *denom, int device_ptrs);
/* common[i] / denom[i] of the pair (i, target[i]) by the pair rule of the distance path, one workgroup per list; the pair
 * (i, i) goes through the rule like any other (common == denom == len[i] for len[i] <= s).  target[i] >= n: MHX_E_ARG,
 * checked on the host in both forms; the other checks are mhx_dist_medoids'. */
int mhx_dist_to(const uint64_t *rows, const uint32_t *len, uint32_t n, uint32_t stride, int k, uint32_t s, const uint32_t *target,
                uint32_t *common, uint32_t *denom, int device_ptrs);
uint64_t mhx_last_medoid_blocks(void);
/* The dereplication at file level for every linkage, with the distance of every member to its representative: the set is
 * read as mhx_cluster_files reads it; the labels come from mhx_dist_cluster (linkage 0, single) or from mhx_dist_linkage cut
 * by mhx_linkage_labels (1 complete, 2 average) at max_dist; the representative of a cluster is its first (rep 0) or its
 * longest member (rep 1) as there, or its medoid (rep 2, mhx_dist_medoids).  One row per reference, clusters and members
 * ordered as mhx_cluster_files orders them:
 *     cluster\tsize\trepresentative\tmember\tdist\tp\tcommon/denom\n
 * dist, p and common/denom as the edge row of mhx_triangle_files prints them, for the pair (member, representative), which
 * mhx_dist_to computes.  out_msh as in mhx_cluster_files, the refusal for multiplicity counts included.  opts == NULL means
 * {sizeof, 0, 0, 2, 1.0}.  MHX_E_ARG: struct_size != sizeof(mhx_cluster_reps_opts), linkage outside 0 .. 2, rep outside
 * 0 .. 2, a max_dist that is not a number.  Pinned by the restated rule (tests/medoid_rule.py).  Not built: a p-value filter. */
typedef struct mhx_cluster_reps_opts {
    uint32_t struct_size; /* sizeof(mhx_cluster_reps_opts) */
    int32_t comment;      /* non-zero: print comments in place of names */
    int32_t linkage;      /* 0 single, 1 complete, 2 average */
    int32_t rep;          /* 0 first, 1 longest, 2 medoid */
    double max_dist;      /* the bound of the clustering */
} mhx_cluster_reps_opts;
int mhx_cluster_reps_files(const char *const *msh_paths, int n_paths, const mhx_cluster_reps_opts *opts, const char *out_msh, char *stdout_buf,
                           size_t cap, size_t *need);

/* Single-linkage TREE of ONE set: the minimum spanning tree of the graph of all pairs, which is the single-linkage
 * dendrogram -- its n - 1 edges, sorted, are the merges, and cutting them at any D gives the clusters of mhx_dist_cluster at
 * D (mhx_mst.h: mst_labels; engine.mst_labels in Python).  rows / len / n / stride / k / s as mhx_dist_triangle takes them,
 * with its checks (n > 65 536, k, s, stride, len[i] > stride, null pointers: MHX_E_ARG); in addition s >= 2^20 is MHX_E_ARG.
 * All before anything is launched.  n == 0 and n == 1: MHX_OK, no edge.
 * Pairs: every pair j < i is an edge with the (common, denom) of mhx_dist_triangle; no distance bound applies.
 * Edge order: edge a precedes edge b iff its Jaccard index common / denom is greater, compared exactly (a.common * b.denom >
 * b.common * a.denom in 64 bits; common == denom counts as 1/1, 0/0 included); equal indices go by the lower min(i, j), then
 * by the lower max(i, j).  The order is total and strict, so the tree is unique: Kruskal over the edges in this order.
 * Outputs, [n - 1] each: edge_i > edge_j the ends, common / denom of the pair, dist (may be NULL) its distance.
 * Host pointers: the edges come out in edge order -- the merge order of the dendrogram -- and dist is host libm, the double
 * mhx_dist_triangle gives.  device_ptrs != 0 => rows, len and the five outputs are device pointers; the edge SET is exact and
 * the same from run to run, the order is that of arrival and unspecified, dist is the device's log.
 * Boruvka on the device: every round each component picks its best outgoing edge in the edge
 * order -- pairs propose to a 64-bit word per list with a compare-and-swap loop, lists to a 32-bit word per component --, the
 * picks join the lock-free union-find of the clustering, one small readback per round tells the host how many components
 * are left.  At most ceil(log2 n) + 1 rounds (more: MHX_E_INTERNAL); mhx_last_mst_rounds() reports the rounds of the last
 * call.  The pairs of a round come from the packed triangle, computed once, when its 8 n (n - 1) / 2 bytes fit
 * MHX_MST_STORE_MB (default 4096: n <= 32 768) -- the only thing of size n^2 this call ever holds, released on return -- and
 * from the triangle's blocks run again every round otherwise (workspace O(n)); MHX_MST_STORE=0|1 forces either form.
 * mhx_last_mst_stored() reports the form that ran: 1 stored, 0 recomputed, -1 when the last call launched nothing.
 * Geometry, MHX_TRI_GEOMETRY and MHX_TRI_QBATCH are the triangle's, and its three diagnostics report this call too, with
 * these meanings: mhx_last_dist_kernel_ms is stream time, the readbacks between rounds included -- stored: the triangle's own
 * figure plus the time from the first launch of the rounds to the last; recomputed: from the first launch of the triangle's
 * passes (behind the set-up of parent and comp, which is not in it) to the last of the last round.
 * mhx_last_dist_fallback_blocks counts the blocks the generic kernel redid ONCE: those of the triangle (stored), those of the
 * FIRST round (recomputed, where every later round redoes the same blocks again without counting them).
 * mhx_last_dist_ranges is the triangle's.  Not built: a sorted device form, more than 65 536 lists (average and complete linkage:
 * mhx_dist_linkage below). */
int mhx_dist_mst(const uint64_t *rows, const uint32_t *len, uint32_t n, uint32_t stride, int k, uint32_t s, uint32_t *edge_i,
                 uint32_t *edge_j, uint32_t *common, uint32_t *denom, double *dist, int device_ptrs);
int mhx_last_mst_rounds(void);
int mhx_last_mst_stored(void);
/* The cut of that tree at max_dist, on the host (no device needed): a union-find over the n - 1 tree edges whose host libm
 * distance -- the double mhx_dist_triangle gives -- is <= max_dist; label[n], label[i] = the lowest index of i's cluster,
 * *n_clusters their number.  Equal to mhx_dist_cluster's labels at max_dist.  The edges may come in any order (a device-form
 * result copied back as it is).  MHX_E_ARG: null pointers, k outside 1 .. 32, a max_dist that is not a number, an edge end
 * >= n.  n == 0: MHX_OK, 0 clusters. */
int mhx_mst_labels(const uint32_t *edge_i, const uint32_t *edge_j, const uint32_t *common, const uint32_t *denom, uint32_t n, int k,
                   double max_dist, uint32_t *label, uint32_t *n_clusters);
/* The same at file level: the references of all files form one set, read and checked as mhx_triangle_files does (k / seed /
 * sketch-size mismatches MHX_E_MISMATCH, damaged files, at most 65 536 references; sketch sizes from 2^20: MHX_E_ARG).
 * Default output, one row per merge in merge order (names; comments when `comment` is set):
 *     name_i\tname_j\tdist\tp\tcommon/denom\tclusters\n
 * the first five fields are the edge-list row of mhx_triangle_files for the pair, `clusters` the number of clusters left after
 * this merge (n - 1 down to 1).  newick != 0 prints the dendrogram instead: the height of a node is its merge distance, a
 * branch is as long as the parent is higher than the child (leaves at 0), floored at 0 and printed %g; of two children the
 * one whose lowest reference index is lower comes first; a name is single-quoted when it holds any of ( ) [ ] ' : ; , or a
 * blank, an inner quote doubled; one reference prints "name;", the output ends ";\n".  opts == NULL means {sizeof, 0, 0}.
 * MHX_E_ARG: struct_size != sizeof(mhx_tree_opts).  Not pinned by mash output (mash has no such command): pinned by the
 * restated rules (tests/mst_rule.py, tests/tree_rule.py), its pairs by the mash-pinned distance path. */
typedef struct mhx_tree_opts {
    uint32_t struct_size; /* sizeof(mhx_tree_opts) */
    int32_t comment;      /* non-zero: print comments in place of names */
    int32_t newick;       /* non-zero: the dendrogram in Newick format in place of the merge table */
} mhx_tree_opts;
int mhx_tree_files(const char *const *msh_paths, int n_paths, const mhx_tree_opts *opts, char *stdout_buf, size_t cap, size_t *need);

/* COMPLETE- and AVERAGE-linkage agglomeration of ONE set (linkage = 1 complete, 2 average; single linkage is mhx_dist_mst):
 * rows / len / n / stride / k / s as mhx_dist_triangle takes them, with its checks (n > 65 536, k, s, stride, len[i] > stride,
 * null pointers: MHX_E_ARG), s >= 2^20, another linkage value or a null output (dist excepted): MHX_E_ARG, all before anything
 * is launched.  n == 0 and n == 1: MHX_OK, nothing written.
 * Clusters carry the index of their lowest member.  Every step merges the pair of clusters with the smallest linkage value,
 * among equal values the pair with the lower `lo` id, then the lower `hi` id; the merged cluster keeps id lo.  n - 1 steps.
 *   complete: the value of a cluster pair is the (common, denom) of its worst leaf pair -- the smallest Jaccard index, compared
 *             exactly as mhx_dist_mst compares (common == denom counts as 1/1); of two equal indices the greater denom stays.
 *   average:  the exact rational num / den, num the sum over all leaf pairs of the fixed-point distance q (below), den = |A| |B|,
 *             compared by the cross products in 128 bits (UPGMA).
 * Outputs, [n - 1] each, in merge order in both pointer forms: merge_a > merge_b the two ids, size the members after the
 * merge, num / den the value (complete: common / denom of the decisive pair), dist (may be NULL) the height -- complete: the
 * distance mhx_dist_triangle gives for the decisive pair; average: ((double)num / (double)den) * 2^-32.  Host pointers: dist is
 * host arithmetic (libm for complete).  device_ptrs != 0 => rows, len and the six outputs are device pointers; every integer
 * output is exact and the same from run to run, dist is the device's arithmetic.
 * On the device: the packed triangle of mhx_dist_triangle's dense mode becomes one 64-bit word per
 * cluster pair; a step is three launches -- one workgroup picks among the rows' cached nearest partners, one thread per
 * cluster combines its two words, the rows that lost their cached partner are scanned again -- and the host enqueues all steps
 * without reading anything back between them.  Memory: 8 n (n - 1) / 2 bytes of words for the whole call plus as many for the
 * triangle's two arrays until the words are made (peak 16 n (n - 1) / 2 bytes).  The words must fit MHX_LINKAGE_STORE_MB
 * (default 4096: n <= 32 768), otherwise MHX_E_CAPACITY; there is no recomputed form.  mhx_last_linkage_rescans() reports the rows
 * scanned again by the steps of the last call; the mhx_last_dist_* diagnostics report the triangle plus the steps.
 * Neighbour joining: mhx_dist_nj below.  Not built: Ward, a recomputed pair source, a p-value column, more than 65 536 lists. */
int mhx_dist_linkage(const uint64_t *rows, const uint32_t *len, uint32_t n, uint32_t stride, int k, uint32_t s, int linkage,
                     uint32_t *merge_a, uint32_t *merge_b, uint32_t *size, uint64_t *num, uint64_t *den, double *dist, int device_ptrs);
int mhx_last_linkage_rescans(void);
/* The cut of those merges at max_dist, on the host (no device needed): the merges from the first one on while dist[t] <=
 * max_dist, none behind the first that is not; label[n], label[i] = the lowest index of i's cluster.  Returns the number of
 * clusters, or a negative MHX_E_* code (MHX_E_ARG: null pointers, a max_dist that is not a number, a merge that does not name
 * ids merge_b < merge_a < n).  With complete linkage every two members of a cluster are within max_dist of each other. */
int64_t mhx_linkage_labels(const uint32_t *merge_a, const uint32_t *merge_b, const double *dist, uint32_t n, double max_dist, uint32_t *label);
/* The fixed-point distance of average linkage in units of 2^-32, integers alone (mhx_linkage.h), on the host: 0 for common ==
 * denom, 2^32 for common == 0, else min(2^32, floor(floor(log2((common + denom) / (2 common)) * 2^40) * floor(ln 2 * 2^32) / 2^40) / k);
 * within 4 units of the distance mhx_dist_triangle gives.  common > denom, denom >= 2^21 or k outside 1 .. 32: UINT64_MAX. */
uint64_t mhx_linkage_fixed_distance(uint32_t common, uint32_t denom, int k);
/* The same at file level: the set is read and checked as mhx_tree_files reads it.  mode 0, one row per merge in merge order:
 *     name_a\tname_b\tdist\tsize\tclusters\n
 * the names of the two ids (comments when `comment` is set), the height as the triangle prints a distance, the members of the
 * merged cluster and the clusters left.  mode 1: the Newick dendrogram by the rules of mhx_tree_files.  mode 2: the cut at
 * max_dist, one row per reference, clusters and members ordered as mhx_cluster_files orders them:
 *     cluster\tsize\trepresentative\tmember\n
 * rep and out_msh as there (out_msh in mode 2 only), the refusal for multiplicity counts included; no degree column: nothing
 * here computes neighbours.  opts == NULL means {sizeof, 0, 1, 0, 0, 1.0}.  MHX_E_ARG: struct_size != sizeof(mhx_linkage_opts),
 * linkage outside 1 .. 2, mode outside 0 .. 2, rep outside 0 .. 1, a max_dist that is not a number, out_msh outside mode 2. */
typedef struct mhx_linkage_opts {
    uint32_t struct_size; /* sizeof(mhx_linkage_opts) */
    int32_t comment;      /* non-zero: print comments in place of names */
    int32_t linkage;      /* 1 complete, 2 average */
    int32_t mode;         /* 0 merge table, 1 Newick, 2 the cut at max_dist */
    int32_t rep;          /* mode 2: 0 first, 1 longest */
    double max_dist;      /* mode 2: merges up to this height */
} mhx_linkage_opts;
int mhx_linkage_files(const char *const *msh_paths, int n_paths, const mhx_linkage_opts *opts, const char *out_msh, char *stdout_buf,
                      size_t cap, size_t *need);

/* NEIGHBOUR JOINING over ONE set: the unrooted tree of the distances of all pairs.  rows / len / n / stride / k / s as
 * mhx_dist_triangle takes them, with its checks (n > 65 536, k, s, stride, len[i] > stride, null pointers: MHX_E_ARG), s >= 2^20
 * or a null output (len_a and len_b excepted, which may both be NULL): MHX_E_ARG, all before anything is launched.  n == 0 and
 * n == 1: MHX_OK, nothing written.
 * The rule, all of it in integers: d(i, j) of two leaves is mhx_linkage_fixed_distance of the pair, in units of 2^-32.  A node
 * carries the id of its lowest leaf; m = n nodes are active at the start; r_i is the sum of d(i, c) over the active c != i.
 * While m > 2 the pair with the smallest Q(i, j) = (m - 2) d(i, j) - r_i - r_j (signed 64 bits) joins, among equal Q the pair with
 * the lower `lo` id, then the lower `hi` id.  With b < a, b becomes the new node u and a dies; for every other active c
 *     d(u, c) = max(0, (d(a, c) + d(b, c) - d(a, b)) >> 1)          (floor)
 * r_c += d(u, c) - d(a, c) - d(b, c), and r_u is the sum of the d(u, c).  The clamp at 0 is a deliberate deviation from
 * textbook neighbour joining, which lets negative distances stand: it keeps every distance in 0 .. 2^32.  On an additive matrix
 * it never acts; mhx_last_nj_clamps() reports how many updates of the last call it changed.
 * Outputs, [n - 1] each, in join order and the same bytes in both pointer forms: join_a > join_b the two ids, d their distance
 * and r_a, r_b their sums, all as they were before the join (join t is made with m = n - t nodes active); the last record joins
 * the two nodes that are left and has r_a = r_b = 0.  len_a, len_b (both or neither NULL), the branch lengths, for m > 2:
 *     len_a = (double)(d (m - 2) + r_a - r_b) / (double)(2 (m - 2)) * 2^-32,   len_b the same with r_a and r_b swapped
 * -- integers below 2^53, one division: every host and the device give the same double -- and len_a = d * 2^-32, len_b = 0 in
 * the last record.  Lengths may be negative and are reported as computed.  device_ptrs != 0 => rows, len and the outputs are
 * device pointers.
 * On the device: the packed triangle of mhx_dist_triangle's dense mode becomes one 64-bit word per
 * pair; a join is three launches -- a scan of the words of the active rows in equal spans of words, one workgroup that reduces
 * the spans' candidates and writes the record, one thread per node for the update -- and the host enqueues all joins without
 * reading anything back between them.  O(n^3) words are read in all.  Memory and MHX_LINKAGE_STORE_MB as for mhx_dist_linkage
 * (MHX_E_CAPACITY); the mhx_last_dist_* diagnostics report the triangle plus the joins.
 * Not built: an exact pruning of the scan, a recomputed pair source, more than 65 536 lists. */
int mhx_dist_nj(const uint64_t *rows, const uint32_t *len, uint32_t n, uint32_t stride, int k, uint32_t s, uint32_t *join_a, uint32_t *join_b,
                uint64_t *d, uint64_t *r_a, uint64_t *r_b, double *len_a, double *len_b, int device_ptrs);
uint64_t mhx_last_nj_clamps(void);
/* The same at file level: the set is read and checked as mhx_tree_files reads it.  newick == 0, one row per join in join order:
 *     name_a\tname_b\tlen_a\tlen_b\tdist\tnodes\n
 * the names of the two ids (comments when `comment` is set), the two branch lengths and dist = d * 2^-32 as the triangle prints
 * a distance, and the nodes left after the join.  newick != 0: the UNROOTED tree.  Every join but the last is a node
 * "(X:len,Y:len)"; for n >= 3 the root is the trifurcation of the two children of join n - 3 and the node that is left, the
 * latter with the dist of the last join as its length; children in the order of their lowest leaf; lengths "%g" of max(0, len);
 * names quoted as mhx_tree_files quotes them.  n == 2: "(name0:0,name1:d);", n == 1: "name;", n == 0: an empty text. */
int mhx_nj_files(const char *const *msh_paths, int n_paths, int comment, int newick, char *stdout_buf, size_t cap, size_t *need);

/* JACKKNIFE SUPPORT of the neighbour-joining tree: which of its splits survive the sampling noise of the sketch hashes.
 * The rule (auriclass_amd/csrc/mhx_resample.h, restated in tests/resample_rule.py and tests/nj_support_rule.py), all of it in
 * integers.  A hash h is kept in replicate r (0-based) of a call with seed `seed` iff (z >> 32) < T, arithmetic mod 2^64:
 *     z = h + seed + (r + 1) * 0x9E3779B97F4A7C15;  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9;
 *     z = (z ^ (z >> 27)) * 0x94D049BB133111EB;     z ^= z >> 31
 * with T = floor(keep * 2^32) from the double keep, 0 < keep <= 1.  The decision depends on the hash alone: two lists that share
 * a hash keep it both or drop it both.  List i of the replicate is the kept hashes of list i, in order; a list with len[i] == s
 * is full, a shorter one a complete set; s_r is the smallest kept count among the full lists (s when none is full) and every
 * list is cut to its first min(kept, s_r) hashes, which makes each a bottom-s_r sketch.  s_r == 0: MHX_E_ARG, the message names
 * the replicate and keep.  The replicate's tree is the rule of mhx_dist_nj over these lists at sketch size s_r, the same k.
 * The leaf set of the node of join t is the union of those of its two ids; canon(X) = X if leaf 0 is not in X, else its
 * complement; the splits of a tree are canon of the leaf sets of its n - 1 joins.  support[t] of the main tree (the records
 * mhx_dist_nj gives) is the number of replicates whose splits hold canon(leaf set of join t); a split with 0, 1, n - 1 or n
 * leaves on a side is in every tree and gets `replicates`.
 *
 * mhx_resample_rows: one replicate of a set.  out_rows [n][stride] receives the cut lists, zero behind out_len[i] up to the
 * stride (another place than rows), *s_out (HOST in both forms) s_r.  device_ptrs != 0 => rows, len, out_rows and out_len are
 * device pointers.  MHX_E_ARG before anything is launched: keep outside (0, 1] or not a number, n > 65 536, s or stride 0, a
 * null pointer, len[i] > stride (host form).  n == 0: MHX_OK, *s_out = s.
 * On the device: one workgroup per row, chunks of 256 hashes, the keep flags of a wave as one ballot, an item's place from the
 * set bits below its lane and the waves' totals through LDS; the full rows fold their count into one word (atomicMin); a second
 * launch cuts every row to it and zeroes the rest. */
int mhx_resample_rows(const uint64_t *rows, const uint32_t *len, uint32_t n, uint32_t stride, uint32_t s, uint64_t seed, uint32_t replicate,
                      double keep, uint64_t *out_rows, uint32_t *out_len, uint32_t *s_out, int device_ptrs);
/* The main tree exactly as mhx_dist_nj gives it (the same checks, the same seven outputs in both pointer forms, the same
 * mhx_last_nj_clamps), then `replicates` jackknife trees and the support of every join of the main tree.  HOST pointers in both
 * forms: support [n - 1]; rep_join_a, rep_join_b [replicates][n - 1] (both or neither NULL), the joins of every replicate;
 * rep_s [replicates] (may be NULL), its s_r.  device_ptrs != 0 => rows, len and the seven main-tree outputs are device pointers.
 * MHX_E_ARG before anything is launched: whatever mhx_dist_nj refuses, keep outside (0, 1] or not a number, replicates > 10 000,
 * a NULL support with replicates > 0.  n <= 1: MHX_OK, nothing written.  replicates == 0: the main tree only, support untouched.
 * n == 2: support[0] = replicates.
 * On the device: the rows are staged once; the pair words, the triangle's two arrays, the state of the
 * joins and one replicate row matrix are allocated once.  A replicate is resample, cut, one 4-byte readback of s_r, dense
 * triangle, init and joins, and the copy of its join_a / join_b to the host, where its splits are counted at once (bitsets,
 * compared exactly; n^2 / 8 bytes of host memory for the main tree's).  Memory: 16 n (n - 1) / 2 bytes for the whole call -- the
 * triangle's arrays stay -- and a second row matrix; the words must fit MHX_LINKAGE_STORE_MB (MHX_E_CAPACITY).  The
 * mhx_last_dist_* time is the sum over the main tree and all replicates.
 * Not built: support for the linkage trees, one batched launch for many small replicates, Felsenstein's bootstrap (which
 * sketches resampled sequence again). */
int mhx_dist_nj_support(const uint64_t *rows, const uint32_t *len, uint32_t n, uint32_t stride, int k, uint32_t s, uint32_t replicates, double keep,
                        uint64_t seed, uint32_t *join_a, uint32_t *join_b, uint64_t *d, uint64_t *r_a, uint64_t *r_b, double *len_a, double *len_b,
                        uint32_t *support, uint32_t *rep_join_a, uint32_t *rep_join_b, uint32_t *rep_s, int device_ptrs);
/* The count alone, on the host (no device needed): support [n - 1] of the joins join_a / join_b [n - 1] among the trees
 * rep_join_a / rep_join_b [replicates][n - 1], exact (bitsets).  n <= 1: MHX_OK, nothing written.  MHX_E_ARG: null pointers,
 * n > 65 536, joins that are no tree of n leaves (ids b < a < n, both nodes at the time of the join). */
int mhx_nj_split_support(const uint32_t *join_a, const uint32_t *join_b, const uint32_t *rep_join_a, const uint32_t *rep_join_b, uint32_t n,
                         uint32_t replicates, uint32_t *support);
/* mhx_nj_files with support values.  replicates == 0 prints exactly what mhx_nj_files prints.  replicates = R > 0: the table
 * gets a seventh column "c/R", c the support of the join; in the Newick text the node of every join t <= n - 4 (the inner nodes
 * but the root) carries the label floor(100 c / R) between ")" and ":", as in "(A:0.1,B:0.2)87:0.05".  The trifurcation carries
 * none: the split of join n - 3 is that of the branch of its third child.  opts == NULL means {sizeof, 0, 0, 0, 0.5, 42}.
 * MHX_E_ARG: struct_size != sizeof(mhx_nj_opts), and what mhx_dist_nj_support refuses.  Pinned by the restated rules
 * (tests/nj_rule.py, tests/nj_support_rule.py). */
typedef struct mhx_nj_opts {
    uint32_t struct_size; /* sizeof(mhx_nj_opts) */
    int32_t comment;      /* non-zero: print comments in place of names */
    int32_t newick;       /* non-zero: the unrooted tree in Newick format in place of the table of joins */
    uint32_t replicates;  /* jackknife replicates, 0: none */
    double keep;          /* the share of the hashes a replicate keeps, (0, 1] */
    uint64_t seed;
} mhx_nj_opts;
int mhx_nj_files_opts(const char *const *msh_paths, int n_paths, const mhx_nj_opts *opts, char *stdout_buf, size_t cap, size_t *need);

/* Reference-set search: for every query the `top` (1 .. 64) closest references whose distance is <= max_dist, ranked and
 * filtered on the device; no [nq][nr] array exists anywhere and nq * nr is not limited.  q / q_len / r / r_len / stride as
 * mhx_dist_batch takes them, (common, denom) of a pair are mhx_dist_batch's.
 * Rank: by the Jaccard index common / denom compared exactly -- a before b iff a.common * b.denom > b.common * a.denom in
 * 64-bit integers, common == denom counting as 1/1 (which includes 0/0, two empty lists: distance 0) -- and pairs of equal
 * index by the lower reference index: a total order.  Not by the distance, which is clamped to 1.
 * Filter: a pair is a hit when the distance mhx_dist_batch computes on the host (libm) is <= max_dist; max_dist >= 1 keeps all.
 * Outputs: hit_ref / hit_common / hit_denom / hit_dist are [nq][top] row-major, best first, n_hits[nq] the hits of each
 * query (min(top, hits)); hit_dist may be NULL.
 * Host pointers: exact by the rule above (the device prefilters by the Jaccard index of max_dist lowered by 2^-30 relative,
 * as mhx_dist_triangle_edges does; the host applies the libm rule to the lists -- a pair it drops ranks behind all it keeps);
 * distances are host libm doubles; entries behind n_hits[q] are zero.
 * device_ptrs != 0: all pointers are device pointers, the lists stay on the device: prefiltered only (see
 * mhx_dist_triangle_edges), still in rank order, hit_dist the device's log, entries behind n_hits[q] unspecified.
 * max_dist < 0: no distance is negative, so the host form returns no hit at all; the prefilter takes such a bound for 0, so
 * the device form's lists are those of max_dist = 0 -- the pairs with common == denom, distance 0.
 * nq == 0 or nr == 0: MHX_OK, n_hits zeroed where there are queries.  MHX_E_ARG: top outside 1 .. 64, max_dist not a
 * number, k outside 1 .. 32, s or stride zero, a len > stride (host form), a null required pointer.
 * Both sets are split into value ranges once per call with one shift; reference slices of 32 lists and query batches form
 * the blocks, a block's candidates are merged into the queries' best lists by one wave per query.
 * Ranges as mhx_dist_triangle (64 at s = 1000); MHX_SEARCH_GEOMETRY=dist takes mhx_dist_batch's geometry, MHX_SEARCH_QBATCH
 * bounds the queries of a block.  mhx_last_dist_kernel_ms, mhx_last_dist_fallback_blocks and mhx_last_dist_ranges report
 * this call too. */
int mhx_dist_search(const uint64_t *q, const uint32_t *q_len, uint32_t nq, const uint64_t *r, const uint32_t *r_len, uint32_t nr,
                    uint32_t stride, int k, uint32_t s, double max_dist, uint32_t top, uint32_t *hit_ref, uint32_t *hit_common,
                    uint32_t *hit_denom, double *hit_dist, uint32_t *n_hits, int device_ptrs);
/* The same at file level: for every query sketch, in argument order and then file order, its hits best first as `mash dist`
 * rows "ref\tquery\tdist\tp\tcommon/denom\n" (p = mhx_p_value); a query without hits prints nothing.  opts == NULL means
 * {sizeof, 5, 1, 1}.  max_p_value drops the rows with p > max_p_value from the `top` already chosen by rank and distance:
 * fewer rows may be printed, a lower-ranked pair is never promoted into their place.  k / seed / sketch-size mismatches
 * (MHX_E_MISMATCH) and damaged files as mhx_dist_files_multi; MHX_E_ARG: struct_size != sizeof(mhx_search_opts), top outside
 * 1 .. 64, a bound that is not a number.  The reference file is read, checked and staged once; the queries are processed
 * in batches, so host memory stays bounded whatever n_qry is.  Not pinned by mash output (mash has no such command): pinned
 * by the restated rule (tests/search_rule.py), its pairs by the mash-pinned distance path. */
typedef struct mhx_search_opts {
    uint32_t struct_size; /* sizeof(mhx_search_opts) */
    uint32_t top;         /* hits per query, 1 .. 64 */
    double max_dist;      /* keep pairs with distance <= max_dist (1: all) */
    double max_p_value;   /* print rows with p <= max_p_value (1: all) */
} mhx_search_opts;
int mhx_search_files(const char *ref_msh, const char *const *qry_msh, int n_qry, const mhx_search_opts *opts, char *stdout_buf,
                     size_t cap, size_t *need);

/* ALL REFERENCES WITHIN A DISTANCE OF EACH QUERY, AS CSR: the bounded neighbourhood call -- "which of the references we know
 * lie within max_dist of this sample" -- without the 64-hit ceiling of mhx_dist_search and without a cell per pair; no
 * [nq][nr] array exists anywhere and nq * nr is not limited.  q / q_len / r / r_len / stride as mhx_dist_batch takes them,
 * (common, denom) of a pair are mhx_dist_batch's.
 * Rule: a pair (q, r) is a hit iff the distance mhx_dist_batch computes on the host (libm) is <= max_dist.  max_dist >= 1
 * keeps every pair, max_dist < 0 none; 0/0 (two empty lists) has distance 0.
 * Outputs: the hits of query q are hit_ref / hit_common / hit_denom / hit_dist [row_off[q] .. row_off[q + 1]), ascending by
 * reference index; row_off [nq + 1], row_off[nq] == *n_out (host, always).  hit_dist may be NULL.
 * Exact in both forms: the bound reaches the kernels as the integer table cmin[0 .. s] of mhx_dist_cluster (built on the host
 * with its libm, kept per (s, k, max_dist)), a pair is a hit iff common >= cmin[denom]; there is no prefilter and no host
 * post-filter, and the two forms return the same integers bit for bit.  Host form: hit_dist are host libm doubles;
 * device_ptrs != 0: all pointers but n_out are device pointers, hit_dist is the device's log.
 * Deterministic: the result is the same from run to run, whatever the batch sizes are and whenever a flagged block is redone.
 * Capacity: cap is the room of the hit arrays in entries.  *n_out > cap: MHX_E_CAPACITY; row_off and *n_out are complete and
 * correct then (the hit arrays hold nothing of use), so the caller sizes the arrays exactly and calls once more.
 * hit_ref == NULL with cap == 0 is the counting form: MHX_OK, only row_off and *n_out are written.
 * nq == 0: MHX_OK, nothing written.  nr == 0: MHX_OK, row_off zeroed, *n_out = 0.  MHX_E_ARG, before anything is launched: a
 * null required pointer, max_dist not a number, k outside 1 .. 32, s or stride zero, s >= 2^20, a len > stride (host form).
 * On the device: the schedule of mhx_dist_search; behind every block one half-wave per (query, slice
 * of 32 references) ballots the rule into one mask word and appends its keepers to an arrival list with one atomic per wave;
 * behind the last block a scan of the mask words gives row_off and a gather puts every hit in its final place, so arrival
 * order never shows.  The queries go through in super-batches of at most 2^22 (query, slice) cells (8 bytes each).
 * MHX_WITHIN_GEOMETRY=dist takes mhx_dist_batch's geometry, MHX_WITHIN_QBATCH bounds the queries of a block, MHX_WITHIN_CELLS
 * lowers the cells of a super-batch.  mhx_last_dist_kernel_ms, mhx_last_dist_fallback_blocks and mhx_last_dist_ranges report
 * this call too. */
int mhx_dist_within(const uint64_t *q, const uint32_t *q_len, uint32_t nq, const uint64_t *r, const uint32_t *r_len, uint32_t nr,
                    uint32_t stride, int k, uint32_t s, double max_dist, uint64_t *row_off, uint32_t *hit_ref, uint32_t *hit_common,
                    uint32_t *hit_denom, double *hit_dist, uint64_t cap, uint64_t *n_out, int device_ptrs);
/* The same at file level, `mash dist -d max_dist -v max_p_value REF QUERY [QUERY ...]`: for every query sketch, in argument
 * order and then file order, every reference within max_dist as a `mash dist` row "ref\tquery\tdist\tp\tcommon/denom\n"
 * (p = mhx_p_value); a query without hits prints nothing.  order 0: the hits of a query in reference order, what mash
 * prints; order 1: best first in the order of mhx_dist_search (the host sorts each row of the CSR).  Rows with
 * p > max_p_value are dropped on the host (mash's pass rule: distance <= -d && p <= -v).  opts == NULL means {sizeof, 0, 1, 1}.
 * Mismatches (MHX_E_MISMATCH) and damaged files as mhx_search_files; MHX_E_ARG: struct_size != sizeof(mhx_within_opts), order
 * outside 0 .. 1, a bound that is not a number.  The reference file is read, checked and staged once; the queries go in
 * batches, a batch whose hits exceed its buffers is repeated once with the size the device reported.  No mash output is
 * recorded for this mode: it is pinned by the restated rule (tests/within_rule.py) over the mash-pinned distance path. */
typedef struct mhx_within_opts {
    uint32_t struct_size; /* sizeof(mhx_within_opts) */
    uint32_t order;       /* 0: reference order, 1: best first */
    double max_dist;      /* keep pairs with distance <= max_dist (1: all) */
    double max_p_value;   /* print rows with p <= max_p_value (1: all) */
} mhx_within_opts;
int mhx_within_files(const char *ref_msh, const char *const *qry_msh, int n_qry, const mhx_within_opts *opts, char *stdout_buf,
                     size_t cap, size_t *need);

/* JACKKNIFE SUPPORT OF SEARCH HITS: in how many of `replicates` resampled sketches each of a query's closest references is
 * still the best one.  The rule (auriclass_amd/csrc/mhx_support.h, restated in tests/support_rule.py), all of it in integers.
 * For query q with candidates cand[q][0 .. n_cand[q]) (indices into r; at most top <= 64, distinct) and replicate
 * r = 0 .. replicates - 1: the replicate of the jackknife above (keep function, T, "full" means len == s) over the set
 * [query, candidate 0, ..]; s_r is the smallest kept count among the full lists of THAT set (s when none is full), so it
 * belongs to the query; s_r == 0: MHX_E_ARG, the message names the query, the replicate and keep.  (common, denom) of candidate
 * i are mhx_dist_batch's pair rule over the cut lists at sketch size s_r.  The best candidate of the replicate is the first in
 * the order of mhx_dist_search (exact Jaccard index, common == denom as 1/1, ties by the lower reference index); first[q][i] is
 * the number of replicates whose best candidate is i, so first[q][..] sums to `replicates` for a query with candidates.
 * cand == NULL: candidates 0 .. nr - 1 for every query; needs nr <= 64 and top == nr (n_cand is not read).
 * Outputs: first [nq][top] (entries behind n_cand[q] zero); rep_best [nq][replicates] the reference index of the best candidate,
 * 0xFFFFFFFF for a query without candidates; rep_s [nq][replicates] s_r; rep_common, rep_denom [nq][top][replicates] (entries
 * of candidates behind n_cand[q] unspecified).  Each rep_* may be NULL, rep_common and rep_denom both or neither.
 * device_ptrs != 0 => every pointer is a device pointer; the outputs are the same bytes in both forms.
 * MHX_E_ARG before anything is launched: s or stride 0, top outside 1 .. 64, keep outside (0, 1] or not a number, replicates
 * outside 1 .. 10 000, cand == NULL with nr > 64 or top != nr, a null required pointer (q, q_len, first; r, r_len with nr > 0;
 * n_cand with cand), and in the host form n_cand[q] > top, a candidate >= nr or named twice in a row, a len > stride.  The
 * device form cannot see those: there an index or length that lies is clamped before it is used (n_cand to top, a candidate to
 * nr - 1, a length to the stride), so no load leaves the matrices.  nq == 0: MHX_OK.
 * On the device: given s_r the cut does not change a pair's result, so all replicates of a pair are
 * counted in ONE ascending walk over the distinct values of the two original lists, the replicates on the lanes of a wave
 * and every load the same for all lanes; the merged sequence is cut into one share per wave by merge-path diagonals.  Four
 * launches per batch of queries (kept counts, s_r, pairs, best); nothing is rewritten and one 8-byte word is read back per call.
 * Memory: (3 top + 3) * 4 * replicates bytes of workspace per query of a batch; the queries are cut into batches so that it
 * stays below 256 MiB (MHX_SUPPORT_WORK_MB sets another bound in MiB; a batch holds at least one query, at most 32 768).
 * mhx_last_dist_kernel_ms reports this call too.
 * Not built: a column in AuriClass's report (needs calibration on real isolates), support for `mash dist`, percentile bounds
 * of the replicate distances, kept counts shared between the queries of a common reference set, more than 64 candidates. */
int mhx_dist_support(const uint64_t *q, const uint32_t *q_len, uint32_t nq, const uint64_t *r, const uint32_t *r_len, uint32_t nr,
                     uint32_t stride, uint32_t s, const uint32_t *cand, const uint32_t *n_cand, uint32_t top, uint32_t replicates,
                     double keep, uint64_t seed, uint32_t *first, uint32_t *rep_best, uint32_t *rep_s, uint32_t *rep_common,
                     uint32_t *rep_denom, int device_ptrs);
/* mhx_search_files with support values: files, checks and the search itself as there.  replicates == 0 prints exactly what
 * mhx_search_files prints, and clade_csv must then be NULL (MHX_E_ARG).  replicates = R > 0: the candidates of a query are its
 * hits -- within max_dist, at most top, BEFORE max_p_value drops rows -- and mhx_dist_support runs on them on the device, on the
 * rows the search has staged; every printed row gets a sixth column "c/R", c = first of its reference.  With clade_csv
 * (AuriClass's clade_config.csv: a header line, then "filename,clade" lines split at the last comma) every row gets two more:
 * the clade of its reference and "g/R", g the replicates whose best candidate has that clade.  A reference of REF.msh whose
 * name is no filename of the table: MHX_E_FORMAT, the message names it; a table that cannot be read: MHX_E_IO.
 * opts == NULL means {sizeof, 5, 1, 1, 0, 0.5, 42}.  MHX_E_ARG: struct_size != sizeof(mhx_search_support_opts), and what
 * mhx_search_files and mhx_dist_support refuse.  Pinned by the restated rules (tests/search_rule.py, tests/support_rule.py). */
typedef struct mhx_search_support_opts {
    uint32_t struct_size; /* sizeof(mhx_search_support_opts) */
    uint32_t top;         /* hits per query, 1 .. 64 */
    double max_dist;      /* keep pairs with distance <= max_dist (1: all) */
    double max_p_value;   /* print rows with p <= max_p_value (1: all) */
    uint32_t replicates;  /* jackknife replicates, 0: none */
    double keep;          /* the share of the hashes a replicate keeps, (0, 1] */
    uint64_t seed;
} mhx_search_support_opts;
int mhx_search_files_support(const char *ref_msh, const char *const *qry_msh, int n_qry, const mhx_search_support_opts *opts,
                             const char *clade_csv, char *stdout_buf, size_t cap, size_t *need);

/* CONTAINMENT FROM SKETCHES: which share of each reference's hashes a query holds, read off the two bottom-s lists alone.
 * The rule (auriclass_amd/csrc/mhx_contain.h, restated in tests/contain_rule.py), all of it in integers.  A list is the first
 * min(len, stride, s) entries of its row, ascending and duplicate-free, s the sketch size of ITS set (s_q for q, s_r for r;
 * the two may differ).  A list of s entries is the complete hash set of its input up to its last entry, a shorter one --
 * the empty one too -- is the complete set: bound = the last entry of a list that holds s entries, 2^64 - 1 otherwise.
 * tau = min(bound(query), bound(reference)); up to tau, tau included, both lists are complete, and
 *   n_qry = #{x in query: x <= tau}   n_ref = #{x in reference: x <= tau}   shared = #{x in both: x <= tau}.
 * 2^64 - 1 is a hash like any other; what a row holds behind its list (zeros, the 2^64 - 1 the segmented sketch appends)
 * never counts.  A query whose input contains the reference's input gives shared == n_ref exactly, whatever else it holds:
 * foreign hashes shrink the window, they do not lower the count.  No float is computed on the device; identity and p-value of
 * a pair are mhx_screen_identity(shared, n_ref, k) and mhx_screen_p_value(shared, n_ref, set_size, k) on the host.
 * Outputs: shared / n_qry / n_ref [nq][nr], query-major.  device_ptrs != 0 => every pointer is a device pointer (a result of
 * mhx_sketch_segments goes straight in on either side); the outputs are the same integers in both forms and from run to run.
 * nq == 0 or nr == 0: MHX_OK, nothing is written.  MHX_E_ARG: s_q, s_r or stride zero, a null pointer, and in the host form
 * a len > stride; the device form cannot see the lengths and clips them to the stride and the sketch size.
 * On the device: the schedule of mhx_dist_search -- one split of both sets into value ranges with
 * one shift, reference slices of 32 lists and query batches as blocks, the range pass of mhx_dist_batch -- with a finish pass
 * of its own that sums a pair's byte counters below the range of tau, walks the two slices of that range up to tau and
 * writes the three counts straight into the outputs; a block whose flag went up (a slice above 255 entries, a crowded
 * range: a short list against the full list of a large genome always) is redone by the generic pair kernel, one workgroup
 * per pair, which also serves tiny calls, MHX_DIST_GENERIC and lists above 65 536 entries.  MHX_SEARCH_GEOMETRY and
 * MHX_SEARCH_QBATCH are the search's; mhx_last_dist_kernel_ms, mhx_last_dist_fallback_blocks and mhx_last_dist_ranges
 * report this call too.
 * Not pinned by mash output (mash has no such command): pinned by the restated rule.
 * Not built: the windowed range form (more than 1024 ranges; such lists go to the pair kernel), max-containment and the
 * query-in-reference identity as columns, a containment column in AuriClass's report.tsv (needs calibration).  (The ranked
 * form, a few best references per query in the place of the full table, is mhx_dist_contain_search below.) */
int mhx_dist_contain(const uint64_t *q, const uint32_t *q_len, uint32_t nq, uint32_t s_q, const uint64_t *r, const uint32_t *r_len,
                     uint32_t nr, uint32_t s_r, uint32_t stride, uint32_t *shared, uint32_t *n_qry, uint32_t *n_ref, int device_ptrs);
/* The same at file level: one row per (query sketch, reference sketch), the queries in argument order and then file order,
 * the references of ref_msh in file order:
 *   "reference\tquery\tidentity\tp-value\tshared/n_ref\tshared/n_qry\n"
 * identity = 1 if shared == n_ref > 0, 0 if shared == 0 (also when n_ref == 0), else (shared / n_ref)^(1/k);
 * p = mhx_screen_p_value(shared, n_ref, set_size, k) with set_size the length field of the QUERY sketch (mash stores the
 * estimated set size there for reads, the genome length for assemblies), 1 when n_ref == 0; both printed with %g.  Rows with
 * identity < min_identity or p > max_p_value are dropped; comment != 0 prints the comment fields in place of the names.
 * opts == NULL means {sizeof, 0, 1, 0}.  The k-mer size and the hash seed must be the same in all files and the query files
 * must share one sketch size (MHX_E_MISMATCH, Mash's messages); the sketch size of ref_msh may differ from the queries'.
 * MHX_E_ARG: struct_size != sizeof(mhx_contain_opts), a bound that is not a number, a null path. */
typedef struct mhx_contain_opts {
    uint32_t struct_size; /* sizeof(mhx_contain_opts) */
    int32_t comment;      /* comment fields in place of names */
    double min_identity;  /* print rows with identity >= min_identity (0: all) */
    double max_p_value;   /* print rows with p <= max_p_value (1: all) */
} mhx_contain_opts;
int mhx_contain_files(const char *ref_msh, const char *const *qry_msh, int n_qry, const mhx_contain_opts *opts, char *stdout_buf,
                      size_t cap, size_t *need);

/* WINNER-TAKE-ALL CONTAINMENT: every hash a query shares with the reference set is credited to ONE reference.  Inside a clade
 * the references share almost all their hashes, so the plain counts give one genome near-identical rows for every member;
 * here the best member takes the shared hashes and the others keep what only they hold (`mash screen -w`, for two sets of
 * sketches).  The rule (auriclass_amd/csrc/mhx_contain_winner.h, restated in tests/contain_winner_rule.py), per query q, on top
 * of mhx_dist_contain's list, bound, tau, shared, n_qry and n_ref:
 *   found(q, r)  = {x in list(q) and list(r): x <= tau(q, r)}, so |found(q, r)| = shared(q, r); a value that a reference holds
 *                  only above its own bound, or behind a list's effective length, is not found there
 *   r ranks before r' by the greater exact ratio shared(q, r) / n_ref(q, r) (compared as shared_a * n_ref_b against
 *                  shared_b * n_ref_a in 64 bits), then the greater ref_length[r], then the lower index; a reference with
 *                  n_ref == 0 has found nothing and never competes
 *   winner(q, x) = the best-ranked r with x in found(q, r), for every x found at all
 *   won(q, r)    = #{x in found(q, r): winner(q, x) = r}
 * So won <= shared, won == shared for the best-ranked reference of a query, and the sum of won(q, .) is the number of distinct
 * values found for q.  The ranking differs per query and the window per pair.  2^64 - 1 is a hash like any other and can be won.
 * Outputs won / shared / n_qry / n_ref [nq][nr], query-major; shared, n_qry and n_ref are exactly what mhx_dist_contain writes.
 * ref_length: u64[nr] genome lengths, or NULL (all equal); with device_ptrs != 0 it is a device pointer like every other.
 * Argument rules, no-op cases and the clipping of lengths are mhx_dist_contain's; a null `won` is MHX_E_ARG.  The integers are
 * the same in both forms, from run to run, and whatever the query batch (MHX_SEARCH_QBATCH).
 * On the device: the plain pass as it is, then per query batch over all references a claim pass --
 * one 32-bit winner word per position of a query's list, every pair with shared > 0 walks its two prefixes and proposes
 * r + 1 to the word of every value it found by compare-and-swap, the word moving only to a better-ranked reference -- and a
 * tally of the words into `won`.  Nothing of size nq x nr exists beyond the four outputs.
 * mhx_last_contain_winner_pairs: the pairs the claim pass of the last call walked, that is, the pairs with shared > 0.
 * Not pinned by mash output: pinned by the restated rule.  Not built: see mhx_dist_contain. */
int mhx_dist_contain_winner(const uint64_t *q, const uint32_t *q_len, uint32_t nq, uint32_t s_q, const uint64_t *r,
                            const uint32_t *r_len, uint32_t nr, uint32_t s_r, uint32_t stride, const uint64_t *ref_length,
                            uint32_t *won, uint32_t *shared, uint32_t *n_qry, uint32_t *n_ref, int device_ptrs);
uint64_t mhx_last_contain_winner_pairs(void);
/* mhx_contain_files with winner-take-all rows: the same options, checks, messages and six columns, with `won` in the place of
 * `shared` -- in the identity, in the p-value and in both fractions -- and the filters on those values.  ref_length is the
 * length field of every reference sketch of ref_msh.  The query files go to the device in batches of 4096 sketches; a
 * query's winners depend on that query alone. */
int mhx_contain_files_winner(const char *ref_msh, const char *const *qry_msh, int n_qry, const mhx_contain_opts *opts,
                             char *stdout_buf, size_t cap, size_t *need);

/* CONTAINMENT SEARCH: for every query the `top` (1 .. 64) references it holds the largest share of, ranked on the device --
 * "which of 100 000 known plasmids, marker loci or genomes is IN this sample?" without the [nq][nr] table of
 * mhx_dist_contain.  The Jaccard search (mhx_dist_search) cannot stand in: a plasmid inside a genome has an index near 0 and
 * a containment of 1.  The rule (auriclass_amd/csrc/mhx_contain_search.h, restated in tests/contain_search_rule.py):
 *   candidate(q, r) = (r, shared, n_ref, n_qry), the three integers of mhx_dist_contain for that pair (s_q, s_r: as there)
 *   hit             = shared >= min_shared (>= 1: a pair that shares nothing is never a hit, nor one with n_ref == 0), and
 *                     identity(shared, n_ref, k) >= min_identity, the identity as mhx_contain_files prints it: 1 when
 *                     shared == n_ref, otherwise (shared / n_ref)^(1/k) in host libm doubles.  min_identity > 1: no hits.
 *                     min_shared is there because a one-hash reference inside a tiny window reaches 1/1.
 *   rank            = the larger shared / n_ref first, compared exactly as a 64-bit cross product; on equal shares the
 *                     larger `shared` (200/200 before 3/3); on equal `shared` the lower reference index.  A total order.
 *   result          = per query the first min(top, hits) hits in rank order
 * Outputs hit_ref / hit_shared / hit_n_ref / hit_n_qry [nq][top], query-major, best first, and n_hits [nq].  Host form:
 * entries behind n_hits[q] are zero; device form (device_ptrs != 0: every pointer is a device pointer, a result of
 * mhx_sketch_segments goes straight in on either side): they are unspecified.  The result is exact and identical in both
 * forms and from run to run: the host turns the identity bound into a table of integers with its own libm, need[n] = the
 * least `shared` that is a hit at n_ref = n (n + 1: none) for n = 0 .. min(stride, s_r), and the device only tests
 * shared >= need[n_ref] (as mhx_dist_cluster's distance bound; unlike mhx_dist_search, whose device form is prefiltered only).
 * nq == 0: MHX_OK; nr == 0: MHX_OK and n_hits zeroed.  MHX_E_ARG: top outside 1 .. 64, min_shared == 0, min_identity not a
 * number, k outside 1 .. 32, s_q, s_r or stride zero, a null pointer, and in the host form a len > stride; the device form
 * clips the lengths as mhx_dist_contain does.
 * On the device: the schedule of mhx_dist_contain -- bounds, one split of both sets, (query batch,
 * reference slice) blocks, the range pass, flags read back per group of 4096 blocks -- with the finish pass writing a block's
 * [queries][32] counts block-local and a take-out pass behind every block: one wave64 per query, lane i holding entry i of
 * the query's best list, no atomics.  A flagged block is redone by the pair kernel and taken out then; the total order makes
 * the late arrival harmless.  Tiny calls, MHX_DIST_GENERIC and lists above 65 536 entries go through the pair kernel per
 * block with the same take-out.  Nothing of size nq x nr exists anywhere.  MHX_SEARCH_GEOMETRY and MHX_SEARCH_QBATCH are
 * honoured; mhx_last_dist_kernel_ms, mhx_last_dist_fallback_blocks and mhx_last_dist_ranges report this call too.
 * Not pinned by mash output (mash has no such command): pinned by the restated rule.
 * More than 64 hits per query: mhx_dist_contain_within below.  Not built: the ranking for the winner-take-all form, and what
 * mhx_dist_contain lists. */
int mhx_dist_contain_search(const uint64_t *q, const uint32_t *q_len, uint32_t nq, uint32_t s_q, const uint64_t *r,
                            const uint32_t *r_len, uint32_t nr, uint32_t s_r, uint32_t stride, int k, double min_identity,
                            uint32_t min_shared, uint32_t top, uint32_t *hit_ref, uint32_t *hit_shared, uint32_t *hit_n_ref,
                            uint32_t *hit_n_qry, uint32_t *n_hits, int device_ptrs);
/* The same at file level: for every query sketch, in argument order and then file order, its result as mhx_contain_files
 * rows, best first; the p-value is mhx_screen_p_value at the query's length field.  Rows with p > max_p_value are dropped
 * from the result already chosen -- nothing moves up into their place (mhx_search_files' rule) -- while min_identity and
 * min_shared act before the cut.  A query without hits prints nothing.  opts == NULL means {sizeof, 0, 5, 1, 0, 1}.  Checks
 * and messages are mhx_contain_files's, and top outside 1 .. 64 or min_shared == 0 is MHX_E_ARG.  The reference file is read
 * and staged on the device once; the query files go there in batches of 4096 sketches. */
typedef struct mhx_contain_search_opts {
    uint32_t struct_size; /* sizeof(mhx_contain_search_opts) */
    int32_t comment;      /* comment fields in place of names */
    uint32_t top;         /* hits per query, 1 .. 64 */
    uint32_t min_shared;  /* a hit shares at least this many hashes, >= 1 */
    double min_identity;  /* a hit has identity >= min_identity (0: all) */
    double max_p_value;   /* print rows with p <= max_p_value (1: all) */
} mhx_contain_search_opts;
int mhx_contain_files_search(const char *ref_msh, const char *const *qry_msh, int n_qry, const mhx_contain_search_opts *opts,
                             char *stdout_buf, size_t cap, size_t *need);

/* ALL REFERENCES A QUERY HOLDS, AS CSR: the containment search without its ceiling of 64 hits -- "which of the 100 000
 * plasmids, marker loci or genomes we know are IN this sample, all of them" -- and without a cell per pair; no [nq][nr] array
 * exists anywhere.  A Jaccard bound (mhx_dist_within) cannot stand in, for the reason given at mhx_dist_contain_search.
 * q / q_len / r / r_len / stride / s_q / s_r as mhx_dist_contain takes them, whose three integers a pair's are.
 * Rule (auriclass_amd/csrc/mhx_contain_within.h, restated in tests/contain_within_rule.py): a pair (q, r) is a hit iff it is
 * one for mhx_dist_contain_search -- shared >= min_shared (>= 1) and identity(shared, n_ref, k) >= min_identity in host libm
 * doubles.  min_identity <= 0 keeps every pair that shares at least min_shared hashes, min_identity > 1 none.
 * Outputs: the hits of query q are hit_ref / hit_shared / hit_n_ref / hit_n_qry [row_off[q] .. row_off[q + 1]), ascending by
 * reference index; row_off [nq + 1], row_off[0] == 0, row_off[nq] == *n_out (host, always).
 * Exact in both forms, which return the same integers bit for bit, and the same from run to run, whatever the batch sizes are
 * and whenever a flagged block is redone: the bound reaches the kernels as the need table of mhx_dist_contain_search, there is
 * no prefilter and no host post-filter.  device_ptrs != 0: all pointers but n_out are device pointers (a result of
 * mhx_sketch_segments goes straight in on either side), and lengths the host cannot see are clipped as mhx_dist_contain does.
 * Capacity: cap is the room of the hit arrays in entries.  *n_out > cap: MHX_E_CAPACITY; row_off and *n_out are complete and
 * correct then (the hit arrays hold nothing of use), so the caller sizes the arrays exactly and calls once more.
 * All four hit arrays NULL with cap == 0 is the counting form: MHX_OK, only row_off and *n_out are written; it keeps no
 * arrival list and does no atomic.
 * nq == 0: MHX_OK, nothing written but *n_out = 0.  nr == 0: MHX_OK, row_off zeroed, *n_out = 0.  MHX_E_ARG, before anything
 * is launched: min_shared == 0, min_identity not a number, k outside 1 .. 32, s_q, s_r or stride zero, a null required
 * pointer, a len > stride (host form).
 * On the device: the schedule of mhx_dist_contain_search inside the super-batches of mhx_dist_within;
 * behind every block one half-wave per (query, slice of 32 references) ballots shared >= need[n_ref] into one mask word and
 * appends its keepers (shared, n_ref, n_qry) to an arrival list with one atomic per wave; behind the last block of a
 * super-batch the scan of mhx_dist_within gives row_off and a gather puts every hit in its final place.  Tiny calls,
 * MHX_DIST_GENERIC and lists above 65 536 entries go through the pair kernel per block with the same take-out.
 * MHX_SEARCH_GEOMETRY, MHX_SEARCH_QBATCH and MHX_WITHIN_CELLS are honoured; mhx_last_dist_kernel_ms,
 * mhx_last_dist_fallback_blocks and mhx_last_dist_ranges report this call too.
 * Not pinned by mash output (mash has no such command): pinned by the restated rule.
 * Not built: max-containment or the query-in-reference identity as hit rule, the winner-take-all form, support values, a
 * p-value filter on the device. */
int mhx_dist_contain_within(const uint64_t *q, const uint32_t *q_len, uint32_t nq, uint32_t s_q, const uint64_t *r,
                            const uint32_t *r_len, uint32_t nr, uint32_t s_r, uint32_t stride, int k, double min_identity,
                            uint32_t min_shared, uint64_t *row_off, uint32_t *hit_ref, uint32_t *hit_shared, uint32_t *hit_n_ref,
                            uint32_t *hit_n_qry, uint64_t cap, uint64_t *n_out, int device_ptrs);
/* The same at file level: for every query sketch, in argument order and then file order, EVERY reference it holds as one
 * mhx_contain_files row (the same six columns, the same %g); a query without hits prints nothing.  order 0: the hits of a
 * query in reference order; order 1: best first in the order of mhx_dist_contain_search (the host sorts each row of the CSR).
 * Rows with p > max_p_value are dropped on the host.  opts == NULL means {sizeof, 0, 1, 0, 1, 1}.  Checks and messages are
 * mhx_contain_files_search's; order outside 0 .. 1 or min_shared == 0 is MHX_E_ARG.  The reference file is read, checked and
 * staged on the device once; the query files go there in batches of 4096 sketches with room for 4096 hits at first, and a
 * batch whose hits exceed its buffers is repeated once with the size the device reported (the buffers stay that large). */
typedef struct mhx_contain_within_opts {
    uint32_t struct_size; /* sizeof(mhx_contain_within_opts) */
    int32_t comment;      /* comment fields in place of names */
    uint32_t order;       /* 0: reference order, 1: best first */
    double min_identity;  /* a hit has identity >= min_identity (0: all) */
    uint32_t min_shared;  /* a hit shares at least this many hashes, >= 1 */
    double max_p_value;   /* print rows with p <= max_p_value (1: all) */
} mhx_contain_within_opts;
int mhx_contain_files_within(const char *ref_msh, const char *const *qry_msh, int n_qry, const mhx_contain_within_opts *opts,
                             char *stdout_buf, size_t cap, size_t *need);

/* Segmented sketch: one bottom-s list per segment of ONE dense stream (`mash sketch -i` at buffer level).
 * bytes[n] is an MHX_FMT_SEQ stream, seg_off[n_seg + 1] ascending byte offsets into it (seg_off[n_seg] <= n); segment i is
 * [seg_off[i], seg_off[i + 1]).  A window is k bytes that lie inside ONE segment and are all A/C/G/T (either case); it is
 * hashed as an MHX_FMT_SEQ push hashes it (canonical strand, MurmurHash3_x64_128 seed 42, 32-bit values for k <= 16).
 * Segments may touch: the cut is seg_off, no separator byte is needed between them.
 * rows[n_seg][stride], len[n_seg]: row i receives the min(s, distinct) smallest distinct hashes of segment i, ascending,
 * without multiplicities, len[i] their number -- the layout mhx_dist_batch and mhx_screener_create take, so a result can
 * feed either without leaving the device.  Entries behind len[i] are zero with host pointers and left as they were with
 * device pointers.  n_seg = 0 is MHX_OK; an empty segment or one shorter than k gives len[i] = 0.
 * MHX_E_ARG: k outside 1..32, s = 0, offsets that descend or pass n, stride < min(s, the largest number of k-byte
 * windows of any segment).
 * device_ptrs != 0 => bytes, seg_off, rows and len are device pointers; the stream must be readable from the 4-byte boundary
 * at or before bytes to the next 16-byte boundary past bytes + n (true for any hipMalloc / torch allocation).  Complete
 * when it returns, either way.
 * Segments of at most mhx_sketch_segments_cut() windows are sketched together by one kernel launch (a workgroup each, sort
 * and selection in LDS: exact by construction, no admission threshold); larger ones go one by one through a sketcher on
 * their slice.  With host pointers the stream and the rows are staged on the device in rounds of bounded size. */
int mhx_sketch_segments(const void *bytes, uint64_t n, const uint64_t *seg_off, uint32_t n_seg, int k, uint32_t s,
                        uint64_t *rows, uint32_t *len, uint32_t stride, int device_ptrs);
uint32_t mhx_sketch_segments_cut(void); /* L: the most windows a segment of the one-launch route may hold */

/* scalar pieces of the dist row (host): mash pValue() */
double mhx_p_value(uint64_t common, uint64_t len_ref, uint64_t len_qry, int k, uint64_t denom);

/* ---- containment screen at buffer level -------------------------------------------------- */
typedef struct mhx_screener mhx_screener;

/* The screen table of a reference set, built once on the device: ref_rows is row-major [nr][stride] with ref_len[i]
 * valid, ascending, duplicate-free hashes in row i (values < 2^32 for k <= 16), as mhx_dist_batch takes them;
 * device_ptrs != 0 => both are device pointers.  The rows are copied: the caller's are free when the call returns.
 * s_ref: the sketch size of the reference set (sizes the set-size sketch).  with_set_size != 0: the screener also keeps a
 * bottom-s_ref sketch of everything pushed (a second launch per push over the same bytes); 0: mhx_screener_finish
 * reports a set size of 0 and the caller computes no p-value from it. */
int mhx_screener_create(int k, const uint64_t *ref_rows, const uint32_t *ref_len, uint32_t nr, uint32_t stride, uint32_t s_ref,
                        int with_set_size, int device_ptrs, mhx_screener **out);
void mhx_screener_destroy(mhx_screener *sc);
int mhx_screener_reset(mhx_screener *sc);   /* multiplicities to zero; the table is kept */
/* the contract of mhx_sketcher_push_device / _push_host / _sync (formats, alignment, lifetime of the pushed bytes) */
int mhx_screener_push_device(mhx_screener *sc, const void *d_bytes, uint64_t n, int fmt);
int mhx_screener_push_host(mhx_screener *sc, const void *h_bytes, uint64_t n, int fmt);
int mhx_screener_sync(mhx_screener *sc);
/* shared[nr], median[nr] as in mhx_screen_files, tallied on the device; *set_size (may be NULL) as there, 0 without the
 * set-size sketch.  counts: NULL, or [nr][stride] words that receive the multiplicity of every reference hash (entries
 * beyond ref_len[i] are 0).  MHX_E_CAPACITY when a multiplicity reached the counter's limit (0xF0000000).  May be called
 * again after further pushes. */
int mhx_screener_finish(mhx_screener *sc, uint32_t *shared, uint32_t *median, double *set_size, uint32_t *counts);
/* mhx_screener_finish under winner-take-all (`mash screen -w`): every hash found in the reads is credited to ONE of the
 * references that hold it.  With shared0[i] the plain shared of reference i and n[i] = ref_len[i], the winner of a hash is
 * the holder with the greatest shared0 / n (compared exactly, as shared0[a] * n[b] against shared0[b] * n[a]: the order of
 * the identities, since pow(x, 1 / k) is monotone); among equals the greatest ref_length (genome length; host pointer
 * [nr], NULL = all equal); among equals again the LOWEST INDEX -- Mash walks an unordered_set there and leaves the choice
 * open; this one is ours.  shared[i] = hashes reference i won, median[i] = element [shared / 2] of their ascending
 * multiplicities, counts = the multiplicity where reference i won the entry, 0 elsewhere.  The sum of shared[] is the
 * number of distinct reference hashes found in the reads.  Runs the plain tally, ranks on the host, then a winner pass and
 * the winner tally on the device.  May be called again after further pushes and may alternate with mhx_screener_finish in
 * any order: neither changes what the other reports. */
int mhx_screener_finish_winner(mhx_screener *sc, const uint64_t *ref_length, uint32_t *shared, uint32_t *median, double *set_size,
                               uint32_t *counts);
/* scalar pieces of the screen row (host), Mash's estimateIdentity() and pValueWithin():
 * identity = 1 if shared == n, 0 if shared == 0, else pow(shared / n, 1 / k);
 * p = 1 if shared == 0, else P[Binomial(n, r) >= shared] with r = 1 / (1 + 4^k / floor(set_size)). */
double mhx_screen_identity(uint64_t shared, uint64_t n, int k);
double mhx_screen_p_value(uint64_t shared, uint64_t n, double set_size, int k);

/* .msh container access for callers that hold sketches in memory */
int mhx_msh_write(const char *path, int k, uint32_t s, uint32_t n_refs, const char *const *names,
                  const char *const *comments, const uint64_t *lengths, const uint64_t *const *hashes,
                  const uint32_t *n_hashes);

/* gunzip of an in-memory .gz (all members) with the decoder the FASTQ ingest uses in place of zlib
 * (kseq's gzread inside `mash sketch`, auriclass/classes.py:588).  out == NULL or cap too small:
 * *out_n still receives the inflated size (MHX_E_CAPACITY in the second case). */
int mhx_gunzip_buffer(const void *gz, size_t n, void *out, size_t cap, size_t *out_n);
/* The same with `threads` decoding threads on the first gzip member (block-boundary search, symbolic decoding of the
 * unknown 32 KiB windows, resolution; the result is byte-identical or the call fails); small inputs and threads < 2 take
 * the sequential decoder. */
int mhx_gunzip_buffer_mt(const void *gz, size_t n, void *out, size_t cap, size_t *out_n, int threads);
/* The same on the GPU: all members of the host-resident gzip buffer gz, inflated into DEVICE memory d_out; complete when
 * it returns.  A member is cut into segments (MHX_DINFLATE_SEGMENT compressed bytes apart, default 64 KiB) that the device
 * searches for block starts, decodes symbolically, chains, resolves and checks (CRC-32 per segment, joined on the host,
 * and ISIZE), in rounds that start at 16 segments and double up to 1024 (MHX_DINFLATE_ROUND).  Members go to the device
 * while at least MHX_DINFLATE_MIN (1 MiB) compressed bytes remain from their start and the member before was at least
 * that large; the first smaller member is decoded there too, and what follows it, a BGZF block (bgzip output: its run of
 * blocks goes to the host's block reader) or a header the host decoder refuses go through the host decoders.  Not
 * used by the FASTQ ingest (mhx_sketch_files).
 * The host has the last word: whenever the device path fails (no consistent chain within the pass bound, an invalid
 * code, a CRC or length mismatch, no room) the whole buffer goes through mhx_gunzip_buffer, whose bytes and error are
 * the result -- this call never returns bytes or an error that mhx_gunzip_buffer would not.  d_out == NULL or cap too
 * small: *out_n still receives the inflated size (MHX_E_CAPACITY in the second case).  MHX_E_NO_DEVICE without an engine. */
int mhx_gunzip_device(const void *gz, size_t n, void *d_out, size_t cap, size_t *out_n);
/* the last mhx_gunzip_device: [0] members decoded on the device, [1] segments, [2] segments redone after a false start,
 * [3] resolution hops (segments resolved), [4] compressed bytes handed to the host decoder, [5] inflated bytes, [6] ms of
 * the call (profiling on), [7] reserved (0) */
int mhx_last_inflate_stats(uint64_t *out8);

/* test tool: the device FASTA parser alone (the first half of the FASTA path of mhx_sketch_files and of
 * mhx_sketch_files_individual).  The n bytes of a FASTA in host memory go to the device as they are; the dense sequence
 * stream the sketch kernel would hash (header lines dropped but for their newline, which stays as the one separator byte
 * in front of every record; line breaks, blanks and DEL squeezed out of the sequence lines) comes back in out[0, *total) and
 * the ascending positions of the separators in it in seps[0, *n_seps).  cap or seps_cap too small: *total and *n_seps are
 * still set (MHX_E_CAPACITY).  *relaunches: how often the kernels ran again because the record list had to grow (it only
 * grows within a process).  Returns MHX_OK, a negative MHX_E_* code, or 1 when the file is not for the device parser and
 * the file-level calls take the host record parser: it does not start with '>', or a line starts with '@' or '+'. */
int mhx_fasta_stream(const void *h_bytes, uint64_t n, void *out, uint64_t cap, uint64_t *total,
                     uint64_t *seps, uint64_t seps_cap, uint64_t *n_seps, uint32_t *relaunches);

#ifdef __cplusplus
}
#endif
#endif /* MHX_H */
