// mhx_files_sets.cpp -- the file-level commands over sets of sketches (.msh files): `mash dist` (mhx_dist_files*), `mash
// triangle` (mhx_triangle_files), the dereplication (mhx_cluster_files, mhx_cluster_reps_files), the single-linkage tree (mhx_tree_files), complete
// and average linkage (mhx_linkage_files), neighbour joining (mhx_nj_files) and the reference-set search
// (mhx_search_files), the bounded neighbourhood (mhx_within_files) and the containment from sketches (mhx_contain_files, mhx_contain_files_search, mhx_contain_files_within).  They read sketch files, call the device paths of the engine files and write Mash's text; the ingest
// of sequence files is in mhx_files.cpp.  The commands of query files against one reference file (search, within, contain)
// share their path check, the staging of the references on the device and the walk over the query files in batches
// (set_paths_check, stage_refs, walk_query_files): a command supplies what follows its first query file and what a batch prints.
#include <hip/hip_runtime.h>
#include <ctype.h>
#include <fcntl.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <sys/stat.h>
#include <unistd.h>

#include <algorithm>
#include <chrono>
#include <string>
#include <unordered_map>
#include <vector>

#include "mhx_triangle.h"
#include "mhx_within.h"
#include "mhx_contain_search.h"
#include "mhx_engine_internal.h"
#include "mhx_internal.h"

using namespace mhx;

namespace {

// The options of a command: `o` holds the defaults and takes the caller's struct if there is one.  Its size is its version.
template <class O> int take_opts(const char *cmd, const O *opts, O &o)
{
    if (!opts) return MHX_OK;
    if (opts->struct_size != sizeof(O)) return fail(MHX_E_ARG, "%s: opts->struct_size is not sizeof(mhx_%s_opts)", cmd, cmd);
    o = *opts;
    return MHX_OK;
}

// one row of `mash dist` / `mash triangle -E`; `more`: a further column behind it
void pair_row(std::string &text, const std::string &a, const std::string &b, double dist, double p, uint32_t common, uint32_t denom,
              const std::string &more = std::string())
{
    text += a + "\t" + b + "\t" + fmt_g(dist) + "\t" + fmt_g(p) + "\t" + std::to_string(common) + "/" + std::to_string(denom);
    if (!more.empty()) text += "\t" + more;
    text += "\n";
}

// One more sketch file `x` of a call: k-mer size and hash seed as in `base`, sketch size as in the first file of its kind,
// in Mash's words.
int check_same_kind(const SketchSet &base, const SketchSet &x, uint32_t first_size, const char *first_path, const char *x_path)
{
    if (base.kmer_size != x.kmer_size)
        return fail(MHX_E_MISMATCH, "ERROR: The query and reference sketches have different k-mer sizes (%u and %u)", x.kmer_size, base.kmer_size);
    if (base.hash_seed != x.hash_seed) return fail(MHX_E_MISMATCH, "ERROR: The query and reference sketches have different hash seeds");
    if (x.sketch_size != first_size)
        return fail(MHX_E_MISMATCH, "ERROR: The query sketches %s and %s have different sketch sizes (%u and %u)", first_path, x_path, first_size,
                    x.sketch_size);
    return MHX_OK;
}

// rows of whole 128-byte lines on the device that hold a list of `longest` hashes
uint32_t row_stride(uint32_t longest) { return (std::max<uint32_t>(16, longest) + 15u) & ~15u; }

// the hash lists as the matrix the device calls take: rows [n][stride], zero behind a list's end, and the lengths
void pack_rows(const std::vector<const RefSketch *> &refs, uint32_t stride, std::vector<uint64_t> &rows, std::vector<uint32_t> &len)
{
    const uint32_t n = (uint32_t)refs.size();
    rows.assign((size_t)n * stride, 0);
    len.resize(n);
    for (uint32_t i = 0; i < n; ++i) {
        len[i] = (uint32_t)refs[i]->hash_count();
        if (len[i]) memcpy(&rows[(size_t)i * stride], refs[i]->hash_data(), (size_t)len[i] * 8);
    }
}

// what every `REF QUERY [QUERY ...]` command over resident references checks of its paths, under its own name
int set_paths_check(const char *cmd, const char *ref_msh, const char *const *qry_msh, int n_qry)
{
    if (!ref_msh || !qry_msh || n_qry < 1) return fail(MHX_E_ARG, "%s: a reference sketch path and at least one query sketch path required", cmd);
    for (int i = 0; i < n_qry; ++i)
        if (!qry_msh[i]) return fail(MHX_E_ARG, "%s: query sketch path %d is null", cmd, i);
    return MHX_OK;
}

// The reference set of a call on the device, for all its batches of queries: rows at a stride that holds any list of the call
// (widest_query: the longest a query list gets), every list cut at `cut` entries.  The host's hash lists are released: names
// and lengths stay for the text.  of: the call in the message ("the search").
struct ResidentRefs {
    DevArray<uint64_t> rows;
    DevArray<uint32_t> len;
    SearchRefs refs{nullptr, nullptr, 0, 0, 0};
};
int stage_refs(SketchSet &R, uint32_t cut, uint32_t widest_query, const char *of, ResidentRefs &d)
{
    SearchRefs &refs = d.refs;
    refs.nr = (uint32_t)R.refs.size();
    std::vector<uint32_t> len(refs.nr);
    for (uint32_t i = 0; i < refs.nr; ++i) {
        len[i] = (uint32_t)std::min<size_t>(R.refs[i].hash_count(), cut);
        refs.longest = std::max(refs.longest, len[i]);
    }
    refs.stride = row_stride(std::max(refs.longest, widest_query));
    if (refs.nr == 0) return MHX_OK;
    std::vector<uint64_t> rows((size_t)refs.nr * refs.stride, 0);
    for (uint32_t i = 0; i < refs.nr; ++i) {
        if (len[i]) memcpy(&rows[(size_t)i * refs.stride], R.refs[i].hash_data(), (size_t)len[i] * 8);
        std::vector<uint64_t>().swap(R.refs[i].hashes);
    }
    if (d.rows.grow(rows.size()) != hipSuccess || d.len.grow(refs.nr) != hipSuccess) return fail(MHX_E_HIP, "hipMalloc failed for the reference set of %s", of);
    if (hipMemcpy(d.rows, rows.data(), rows.size() * 8, hipMemcpyHostToDevice) != hipSuccess || hipMemcpy(d.len, len.data(), (size_t)refs.nr * 4, hipMemcpyHostToDevice) != hipSuccess)
        return fail(MHX_E_HIP, "H2D copy of the reference set failed");
    refs.rows = d.rows; refs.len = d.len;
    return MHX_OK;
}

// The query files of a call against the reference file R, read one after the other, so that host memory holds one batch
// whatever n_qry is: every file is checked against R and the first file, on_first_file(Q) follows the first one's check (the
// sizes of the call, the staging of the references), and flush(qs) gets the sketches read so far whenever there are
// kQueryBatch of them, and at the end.  A call without references flushes nothing.
constexpr size_t kQueryBatch = 4096; // query sketches per device call
template <class First, class Flush> int walk_query_files(const SketchSet &R, const char *const *qry_msh, int n_qry, First on_first_file, Flush flush)
{
    std::vector<SketchSet> held; // the files of the current batch
    std::vector<const RefSketch *> qs;
    uint32_t q_sketch_size = 0;
    auto batch = [&]() -> int {
        const int rc = qs.empty() || R.refs.empty() ? MHX_OK : flush(qs);
        qs.clear();
        held.clear();
        return rc;
    };
    for (int i = 0; i < n_qry; ++i) {
        held.emplace_back();
        SketchSet &Q = held.back();
        int rc = msh_read_file(qry_msh[i], Q);
        if (rc) return rc;
        if (i == 0) q_sketch_size = Q.sketch_size;
        rc = check_same_kind(R, Q, q_sketch_size, qry_msh[0], qry_msh[i]);
        if (rc == MHX_OK && i == 0) rc = on_first_file(Q);
        if (rc) return rc;
        for (const RefSketch &q : Q.refs) qs.push_back(&q); // (a SketchSet that moves keeps its references where they are)
        if (qs.size() >= kQueryBatch) { rc = batch(); if (rc) return rc; }
    }
    return batch();
}

// `mash dist REF QUERY [QUERY ...]`: mhx_dist_files is the n_qry == 1 case.  The reference file is read, parsed, checked and
// staged once per call, and the sketches of ALL query files go to the device together, so that a run of samples reaches
// the all-vs-refs kernels in the shape they were made for (many queries x few references) instead of 1 x nr per sample.
int dist_files(const char *ref_msh, const char *const *qry_msh, int n_qry, char *stdout_buf, size_t cap, size_t *need)
{
    int rc = MHX_OK;
    if (n_qry == 1 && (!ref_msh || !qry_msh || !qry_msh[0])) return fail(MHX_E_ARG, "dist: two sketch paths required");
    if (!ref_msh || !qry_msh || n_qry < 1) return fail(MHX_E_ARG, "dist: a reference sketch path and at least one query sketch path required");
    for (int i = 0; i < n_qry; ++i)
        if (!qry_msh[i]) return fail(MHX_E_ARG, "dist: query sketch path %d is null", i);
    // The reference sketch file (9.6 MB at AuriClass's defaults: 24 x 50 000 hashes) is read ONCE, into a pinned block,
    // parsed where it is (64-bit hash lists stay views into the image), checked for order on a few threads and copied
    // row by row from the pinned image into the device staging area: one pass over the bytes on the host instead of
    // five (file buffer, segment copies, hash vectors, padded matrix, pageable H2D staging): 5.6 -> 2 ms per call.
    SketchSet R;
    std::vector<SketchSet> Q((size_t)n_qry);
    std::vector<uint8_t> ref_heap;
    static const bool timing = getenv("MHX_DIST_TIMING") != nullptr; // phase times of a call on stderr
    const auto t_start = std::chrono::steady_clock::now();
    auto lap = [&](const char *what) {
        if (timing) fprintf(stderr, "[mhx dist_files] %s at %.3f ms\n", what, std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t_start).count());
    };
    {
        struct stat sb;
        const int fd = open(ref_msh, O_RDONLY);
        if (fd < 0 || fstat(fd, &sb) != 0 || !S_ISREG(sb.st_mode)) { if (fd >= 0) close(fd); return fail(MHX_E_IO, "cannot open sketch %s", ref_msh); }
        const size_t len = (size_t)sb.st_size;
        uint8_t *img = nullptr;
        if (len >= (1u << 20) && len <= (256u << 20)) { // a pinned block of its own, kept between calls (larger files, or MHX_DIST_PAGEABLE=1: the heap)
            if (g.dist_img.cap() < len && !getenv("MHX_DIST_PAGEABLE") &&
                g.dist_img.grow((len + len / 4 + (1u << 20)) & ~(size_t)((1u << 20) - 1)) != hipSuccess)
                (void)hipGetLastError();
            if (g.dist_img.cap() >= len) img = g.dist_img;
        }
        if (!img) { ref_heap.resize(len); img = ref_heap.data(); }
        const bool ok = len == 0 || parallel_pread(fd, img, 0, len, len >= (4u << 20) ? std::min(8, ingest_thread_budget()) : 1);
        close(fd);
        if (!ok) return fail(MHX_E_IO, "cannot read %s", ref_msh);
        lap("reference file read");
        rc = msh_parse_image(img, len, ref_msh, R, true);
        if (rc) return rc;
        lap("parsed");
        // the distance kernels merge ascending duplicate-free lists (what mash writes); anything else is a damaged file
        std::vector<int> bad(R.refs.size(), 0);
        {
            JoinedThreads th;
            const size_t nthreads = len >= (4u << 20) ? (size_t)std::min(8, ingest_thread_budget()) : 1;
            for (size_t t = 0; t < nthreads; ++t) {
                auto part = [&, t]() {
                    for (size_t i = t; i < R.refs.size(); i += nthreads)
                        if (R.refs[i].view && !check_ascending(R.refs[i].view, R.refs[i].view_n)) bad[i] = 1;
                };
                if (t + 1 == nthreads || !th.spawn(part)) part();
            }
        }
        for (size_t i = 0; i < bad.size(); ++i)
            if (bad[i]) return fail(MHX_E_FORMAT, "%s: hash list of reference %zu is not ascending", ref_msh, i);
        lap("order checked");
    }
    uint64_t nq_all = 0;
    for (int i = 0; i < n_qry; ++i) {
        rc = msh_read_file(qry_msh[i], Q[i]);
        if (rc == MHX_OK) rc = check_same_kind(R, Q[i], Q[0].sketch_size, qry_msh[0], qry_msh[i]);
        if (rc) return rc;
        nq_all += Q[i].refs.size();
    }
    lap("query read");
    const int k = (int)R.kmer_size;
    const uint32_t s = R.sketch_size < Q[0].sketch_size ? R.sketch_size : Q[0].sketch_size;
    const uint32_t nr = (uint32_t)R.refs.size();
    if (nq_all * (nr ? nr : 1) > 0x7FFFFFFFull) return fail(MHX_E_ARG, "too many pairs for one call");
    const uint32_t nq = (uint32_t)nq_all;
    std::string text;
    if (nr && nq) {
        std::vector<const RefSketch *> qs;
        qs.reserve(nq);
        for (const SketchSet &set : Q)
            for (const RefSketch &q : set.refs) qs.push_back(&q);
        std::vector<const uint64_t *> rrows(nr), qrows(nq);
        std::vector<uint32_t> rl(nr), ql(nq);
        for (uint32_t i = 0; i < nr; ++i) { rrows[i] = R.refs[i].hash_data(); rl[i] = (uint32_t)R.refs[i].hash_count(); }
        for (uint32_t i = 0; i < nq; ++i) { qrows[i] = qs[i]->hash_data(); ql[i] = (uint32_t)qs[i]->hash_count(); }
        std::vector<uint32_t> common((size_t)nq * nr), denom((size_t)nq * nr);
        std::vector<double> dist((size_t)nq * nr);
        rc = dist_batch_rows(qrows.data(), ql.data(), nq, rrows.data(), rl.data(), nr, k, s, common.data(), denom.data(), dist.data());
        if (rc) return rc;
        lap("distances back");
        for (uint32_t qi = 0; qi < nq; ++qi)
            for (uint32_t ri = 0; ri < nr; ++ri) {
                const size_t p = (size_t)qi * nr + ri;
                const double pv = mhx_p_value(common[p], R.refs[ri].length, qs[qi]->length, k, denom[p]);
                pair_row(text, R.refs[ri].name, qs[qi]->name, dist[p], pv, common[p], denom[p]);
            }
        lap("text written");
    }
    return put_text(text, stdout_buf, cap, need);
}

// The references of all files as ONE set (argument order, then file order), what `mash triangle`, the clustering and the
// tree start from: every file read and checked, k / seed / sketch size the same in all, at most 65 536 references, and
// their hash lists as the matrix mhx_dist_triangle takes.  `what` names the caller in the messages.
struct SetOfFiles {
    std::vector<SketchSet> F;
    std::vector<const RefSketch *> refs;
    std::vector<uint64_t> rows;
    std::vector<uint32_t> len;
    uint32_t stride = 16;
    uint32_t n() const { return (uint32_t)refs.size(); }
    uint32_t s() const { return F[0].sketch_size ? F[0].sketch_size : 1; } // for the device calls
    int k() const { return (int)F[0].kmer_size; }
};
int read_set_of_files(const char *what, const char *const *paths, int n_paths, SetOfFiles &S)
{
    if (!paths || n_paths < 1) return fail(MHX_E_ARG, "%s: at least one sketch path required", what);
    for (int i = 0; i < n_paths; ++i)
        if (!paths[i]) return fail(MHX_E_ARG, "%s: sketch path %d is null", what, i);
    std::vector<SketchSet> &F = S.F;
    F.resize((size_t)n_paths);
    for (int i = 0; i < n_paths; ++i) {
        int rc = msh_read_file(paths[i], F[i]); // (checks that every hash list ascends: MHX_E_FORMAT)
        if (rc == MHX_OK) rc = check_same_kind(F[0], F[i], F[0].sketch_size, paths[0], paths[i]);
        if (rc) return rc;
        for (const RefSketch &r : F[i].refs) S.refs.push_back(&r);
    }
    if (S.refs.size() > 65536) return fail(MHX_E_ARG, "%s: too many references for one call (%zu)", what, S.refs.size());
    uint32_t longest = 0;
    for (const RefSketch *r : S.refs) longest = std::max<uint32_t>(longest, (uint32_t)r->hash_count());
    S.stride = row_stride(longest);
    pack_rows(S.refs, S.stride, S.rows, S.len);
    return MHX_OK;
}

// Newick: a name is single-quoted when it holds any of ( ) [ ] ' : ; , or a blank, an inner quote doubled
std::string newick_name(const std::string &name)
{
    bool quote = false;
    for (const char ch : name) quote = quote || strchr("()[]':;,", ch) != nullptr || isspace((unsigned char)ch);
    if (!quote) return name;
    std::string out = "'";
    for (const char ch : name) { out += ch; if (ch == '\'') out += ch; }
    return out + "'";
}

// The dendrogram of m = n - 1 merges in merge order (ei / ej: a member, or the id, of either side; dist: the height) as
// Newick: nodes 0 .. n - 1 are the leaves, node n + e the merge e; a node's height is its merge distance (leaves: 0), a branch
// is as long as the parent is higher, never negative; the child whose lowest index is lower comes first.  n >= 1.
template <class Shown>
int newick_text(const char *what, uint32_t n, const std::vector<uint32_t> &ei, const std::vector<uint32_t> &ej, const std::vector<double> &dist, Shown shown,
                std::string &text)
{
    const uint32_t m = n - 1;
    std::vector<uint32_t> top(n), left(m), right(m), lowest((size_t)n + m), find(n);
    std::vector<double> height((size_t)n + m, 0.0);
    for (uint32_t i = 0; i < n; ++i) { top[i] = i; lowest[i] = i; find[i] = i; }
    auto root = [&](uint32_t x) { while (find[x] != x) { find[x] = find[find[x]]; x = find[x]; } return x; };
    for (uint32_t e = 0; e < m; ++e) {
        const uint32_t ra = root(ei[e]), rb = root(ej[e]);
        if (ra == rb) return fail(MHX_E_INTERNAL, "%s: merge %u joins one component with itself", what, e);
        uint32_t a = top[ra], b = top[rb];
        if (lowest[b] < lowest[a]) std::swap(a, b);
        left[e] = a; right[e] = b;
        lowest[n + e] = lowest[a];
        height[n + e] = dist[e];
        find[rb] = ra;
        top[ra] = n + e;
    }
    // written without recursion: a chain of 65 535 merges is a tree of that depth
    struct Item { uint32_t node; int stage; };
    std::vector<Item> todo{{m ? n + m - 1 : 0u, 0}};
    auto branch = [&](uint32_t child, uint32_t parent) { const double d = height[parent] - height[child]; return ":" + fmt_g(d > 0.0 ? d : 0.0); };
    while (!todo.empty()) {
        const Item it = todo.back();
        todo.pop_back();
        if (it.node < n) { text += newick_name(shown(it.node)); continue; }
        const uint32_t e = it.node - n;
        if (it.stage == 0) { text += "("; todo.push_back({it.node, 1}); todo.push_back({left[e], 0}); }
        else if (it.stage == 1) { text += branch(left[e], it.node) + ","; todo.push_back({it.node, 2}); todo.push_back({right[e], 0}); }
        else text += branch(right[e], it.node) + ")";
    }
    text += ";\n";
    return MHX_OK;
}

// out_msh of a clustering is refused when a reference carries what that file cannot store
int check_no_counts(const char *what, const std::vector<const RefSketch *> &refs)
{
    for (const RefSketch *r : refs)
        if (!r->counts.empty())
            return fail(MHX_E_ARG, "%s: %s carries multiplicity counts, which the output sketch file cannot store", what, r->name.c_str());
    return MHX_OK;
}

// A clustering from its labels (label[i]: the lowest member of i's cluster): clusters numbered from 1 by their lowest
// member, their sizes and a representative per cluster in one pass -- the lowest member (rep_rule 0), the member of greatest
// genome length (1), or medoid[i] of any member (2: mhx_dist_medoids) --, O(n).
struct ClusterShape {
    std::vector<uint32_t> number, size, rep, order; // by label: number, members, representative; order: the labels ascending
};
int cluster_shape(const char *what, const SetOfFiles &S, const std::vector<uint32_t> &label, uint32_t n_clusters, int rep_rule, const std::vector<uint32_t> *medoid,
                  ClusterShape &sh)
{
    const std::vector<const RefSketch *> &refs = S.refs;
    const uint32_t n = S.n();
    sh.number.assign(n, 0); sh.size.assign(n, 0); sh.rep.assign(n, 0); sh.order.clear();
    for (uint32_t i = 0; i < n; ++i) {
        const uint32_t l = label[i];
        if (l > i || label[l] != l) return fail(MHX_E_INTERNAL, "%s: label %u of reference %u is not a cluster's lowest member", what, l, i);
        if (l == i) { sh.order.push_back(i); sh.number[i] = (uint32_t)sh.order.size(); sh.rep[i] = rep_rule == 2 ? (*medoid)[i] : i; }
        ++sh.size[l];
        if (rep_rule == 1 && refs[i]->length > refs[sh.rep[l]]->length) sh.rep[l] = i; // members come in index order: ties stay with the lower
    }
    if (sh.order.size() != n_clusters) return fail(MHX_E_INTERNAL, "%s: %zu labels but %u clusters counted", what, sh.order.size(), n_clusters);
    return MHX_OK;
}

// The table of a clustering: members in index order, a row per reference "cluster\tsize\trepresentative\tmember" and what
// column(i) adds behind it (nothing: no further column)
template <class Column> void cluster_rows(const SetOfFiles &S, const std::vector<uint32_t> &label, const ClusterShape &sh, bool comment, Column column, std::string &text)
{
    const std::vector<const RefSketch *> &refs = S.refs;
    const uint32_t n = S.n();
    auto shown = [&](uint32_t i) -> const std::string & { return comment ? refs[i]->comment : refs[i]->name; };
    std::vector<std::vector<uint32_t>> members(sh.order.size());
    for (uint32_t i = 0; i < n; ++i) members[sh.number[label[i]] - 1].push_back(i);
    for (size_t ci = 0; ci < sh.order.size(); ++ci) {
        const uint32_t l = sh.order[ci];
        for (uint32_t i : members[ci]) {
            text += std::to_string(ci + 1) + "\t" + std::to_string(sh.size[l]) + "\t" + shown(sh.rep[l]) + "\t" + shown(i);
            const std::string more = column(i);
            if (!more.empty()) text += "\t" + more;
            text += "\n";
        }
    }
}

// the representatives, unchanged, in cluster order as a sketch file of their own
int cluster_reps_msh(const SetOfFiles &S, const ClusterShape &sh, const char *out_msh)
{
    const uint32_t m = (uint32_t)sh.order.size();
    std::vector<const char *> names(m), comments(m);
    std::vector<uint64_t> lengths(m);
    std::vector<const uint64_t *> hashes(m);
    std::vector<uint32_t> n_hashes(m);
    for (uint32_t ci = 0; ci < m; ++ci) {
        const RefSketch &r = *S.refs[sh.rep[sh.order[ci]]];
        names[ci] = r.name.c_str(); comments[ci] = r.comment.c_str(); lengths[ci] = r.length;
        hashes[ci] = r.hash_data(); n_hashes[ci] = (uint32_t)r.hash_count();
    }
    return mhx_msh_write(out_msh, S.k(), S.F[0].sketch_size, m, names.data(), comments.data(), lengths.data(), hashes.data(), n_hashes.data());
}

// The table of mhx_cluster_files and of the cut of mhx_linkage_files: a row per reference -- with the degree column when there
// are degrees --, and the representatives as a sketch file on request.
int cluster_table(const char *what, const SetOfFiles &S, const std::vector<uint32_t> &label, uint32_t n_clusters, const std::vector<uint32_t> *degree, bool comment,
                  int rep_rule, const char *out_msh, std::string &text)
{
    ClusterShape sh;
    const int rc = cluster_shape(what, S, label, n_clusters, rep_rule, nullptr, sh);
    if (rc) return rc;
    cluster_rows(S, label, sh, comment, [&](uint32_t i) { return degree ? std::to_string((*degree)[i]) : std::string(); }, text);
    return out_msh ? cluster_reps_msh(S, sh, out_msh) : MHX_OK;
}

// The labels of the set at max_dist for mhx_cluster_reps_files: single linkage from mhx_dist_cluster, complete and average from
// the merges of mhx_dist_linkage cut by mhx_linkage_labels
int reps_labels(const SetOfFiles &S, int linkage, double max_dist, std::vector<uint32_t> &label, uint32_t *n_clusters)
{
    const uint32_t n = S.n();
    label.assign(n, 0);
    if (linkage == 0) {
        uint64_t n_edges = 0;
        return mhx_dist_cluster(S.rows.data(), S.len.data(), n, S.stride, S.k(), S.s(), max_dist, label.data(), nullptr, n_clusters, &n_edges, 0);
    }
    const uint32_t m = n ? n - 1 : 0;
    std::vector<uint32_t> ma(m), mb(m), size(m);
    std::vector<uint64_t> num(m), den(m);
    std::vector<double> dist(m);
    const int rc = mhx_dist_linkage(S.rows.data(), S.len.data(), n, S.stride, S.k(), S.s(), linkage, ma.data(), mb.data(), size.data(), num.data(), den.data(),
                                    dist.data(), 0);
    if (rc) return rc;
    const int64_t found = mhx_linkage_labels(ma.data(), mb.data(), dist.data(), n, max_dist, label.data());
    if (found < 0) return (int)found;
    *n_clusters = (uint32_t)found;
    return MHX_OK;
}

} // namespace

extern "C" int mhx_dist_files(const char *ref_msh, const char *qry_msh, char *stdout_buf, size_t cap, size_t *need)
{
    return entry("mhx_dist_files", [&] { return dist_files(ref_msh, &qry_msh, 1, stdout_buf, cap, need); });
}

extern "C" int mhx_dist_files_multi(const char *ref_msh, const char *const *qry_msh, int n_qry, char *stdout_buf, size_t cap, size_t *need)
{
    return entry("mhx_dist_files_multi", [&] { return dist_files(ref_msh, qry_msh, n_qry, stdout_buf, cap, need); });
}

// `mash triangle a.msh [b.msh ...]`: every pair j < i of the set is compared on the device (mhx_dist_triangle, or
// mhx_dist_triangle_edges when a distance bound can drop pairs there), and the text is Mash's CommandTriangle: the
// lower-triangle matrix, or the edge list with its two filters.
extern "C" int mhx_triangle_files(const char *const *paths, int n_paths, const mhx_triangle_opts *opts, char *stdout_buf, size_t cap, size_t *need)
{
    return entry("mhx_triangle_files", [&]() -> int {
        mhx_triangle_opts o{(uint32_t)sizeof(mhx_triangle_opts), 0, 0, 1.0, 1.0};
        int rc = take_opts("triangle", opts, o);
        if (rc) return rc;
        if (!(o.max_dist == o.max_dist) || !(o.max_p_value == o.max_p_value)) return fail(MHX_E_ARG, "triangle: max_dist / max_p_value is not a number");
        const bool edge = o.edge != 0 || o.max_dist < 1.0 || o.max_p_value < 1.0; // -d and -v imply -E
        SetOfFiles S;
        rc = read_set_of_files("triangle", paths, n_paths, S);
        if (rc) return rc;
        const std::vector<const RefSketch *> &refs = S.refs;
        const uint32_t n = S.n();
        const int k = S.k();
        const uint64_t pairs = (uint64_t)n * (n ? n - 1 : 0) / 2;
        std::string text;
        if (!edge) {
            std::vector<uint32_t> common(pairs), denom(pairs);
            std::vector<double> dist(pairs);
            rc = mhx_dist_triangle(S.rows.data(), S.len.data(), n, S.stride, k, S.s(), common.data(), denom.data(), dist.data(), 0);
            if (rc) return rc;
            text = "\t" + std::to_string(n) + "\n";
            for (uint32_t i = 0; i < n; ++i) {
                text += o.comment ? refs[i]->comment : refs[i]->name;
                for (uint32_t j = 0; j < i; ++j) text += "\t" + fmt_g(dist[(size_t)i * (i - 1) / 2 + j]);
                text += "\n";
            }
            return put_text(text, stdout_buf, cap, need);
        }
        std::vector<uint32_t> ei, ej, common, denom;
        std::vector<double> dist;
        uint64_t found = 0, room = o.max_dist >= 1.0 ? pairs : std::min<uint64_t>(pairs, 1u << 16);
        for (int attempt = 0; attempt < 2; ++attempt) {
            ei.resize(room); ej.resize(room); common.resize(room); denom.resize(room); dist.resize(room);
            rc = mhx_dist_triangle_edges(S.rows.data(), S.len.data(), n, S.stride, k, S.s(), o.max_dist, ei.data(), ej.data(), common.data(), denom.data(),
                                         dist.data(), room, &found, 0);
            if (rc != MHX_E_CAPACITY) break;
            room = found;
        }
        if (rc) return rc;
        clear_error();
        for (uint64_t e = 0; e < found; ++e) {
            const RefSketch &a = *refs[ei[e]], &b = *refs[ej[e]];
            const double pv = mhx_p_value(common[e], a.length, b.length, k, denom[e]);
            if (pv <= o.max_p_value) pair_row(text, a.name, b.name, dist[e], pv, common[e], denom[e]);
        }
        return put_text(text, stdout_buf, cap, need);
    });
}

// Dereplication at file level: the references of all files form one set (as for the triangle), mhx_dist_cluster labels it on
// the device, and the host numbers the clusters by their lowest member, picks a representative per cluster in one pass
// and prints a row per reference; the representatives, unchanged, are written as a sketch file of their own on request.
extern "C" int mhx_cluster_files(const char *const *paths, int n_paths, const mhx_cluster_opts *opts, const char *out_msh, char *stdout_buf, size_t cap, size_t *need)
{
    return entry("mhx_cluster_files", [&]() -> int {
        mhx_cluster_opts o{(uint32_t)sizeof(mhx_cluster_opts), 0, 0, 1.0};
        int rc = take_opts("cluster", opts, o);
        if (rc) return rc;
        if (!(o.max_dist == o.max_dist)) return fail(MHX_E_ARG, "cluster: max_dist is not a number");
        if (o.rep != 0 && o.rep != 1) return fail(MHX_E_ARG, "cluster: rep must be 0 (first) or 1 (longest)");
        SetOfFiles S;
        rc = read_set_of_files("cluster", paths, n_paths, S);
        if (rc) return rc;
        const uint32_t n = S.n();
        if (out_msh) { rc = check_no_counts("cluster", S.refs); if (rc) return rc; }
        std::vector<uint32_t> label(n), degree(n);
        uint32_t n_clusters = 0;
        uint64_t n_edges = 0;
        rc = mhx_dist_cluster(S.rows.data(), S.len.data(), n, S.stride, S.k(), S.s(), o.max_dist, label.data(), degree.data(), &n_clusters, &n_edges, 0);
        if (rc) return rc;
        std::string text;
        rc = cluster_table("cluster", S, label, n_clusters, &degree, o.comment != 0, o.rep, out_msh, text);
        if (rc) return rc;
        return put_text(text, stdout_buf, cap, need);
    });
}

// The dereplication with the distance of every member to its representative: labels by the linkage asked for, the
// representative by the rule asked for -- the medoid from mhx_dist_medoids --, the pair (member, representative) of every row
// from mhx_dist_to, printed as the triangle's edge row prints a pair.
extern "C" int mhx_cluster_reps_files(const char *const *paths, int n_paths, const mhx_cluster_reps_opts *opts, const char *out_msh, char *stdout_buf, size_t cap,
                                      size_t *need)
{
    return entry("mhx_cluster_reps_files", [&]() -> int {
        mhx_cluster_reps_opts o{(uint32_t)sizeof(mhx_cluster_reps_opts), 0, 0, 2, 1.0};
        int rc = take_opts("cluster_reps", opts, o);
        if (rc) return rc;
        if (o.linkage < 0 || o.linkage > 2) return fail(MHX_E_ARG, "cluster_reps: linkage must be 0 (single), 1 (complete) or 2 (average)");
        if (o.rep < 0 || o.rep > 2) return fail(MHX_E_ARG, "cluster_reps: rep must be 0 (first), 1 (longest) or 2 (medoid)");
        if (!(o.max_dist == o.max_dist)) return fail(MHX_E_ARG, "cluster_reps: max_dist is not a number");
        SetOfFiles S;
        rc = read_set_of_files("cluster_reps", paths, n_paths, S);
        if (rc) return rc;
        const std::vector<const RefSketch *> &refs = S.refs;
        const uint32_t n = S.n();
        const int k = S.k();
        if (out_msh) { rc = check_no_counts("cluster_reps", refs); if (rc) return rc; }
        std::vector<uint32_t> label, medoid(n), target(n), common(n), denom(n);
        uint32_t n_clusters = 0;
        rc = reps_labels(S, o.linkage, o.max_dist, label, &n_clusters);
        if (rc) return rc;
        if (o.rep == 2) {
            rc = mhx_dist_medoids(S.rows.data(), S.len.data(), n, S.stride, k, S.s(), label.data(), medoid.data(), nullptr, nullptr, nullptr, 0);
            if (rc) return rc;
        }
        ClusterShape sh;
        rc = cluster_shape("cluster_reps", S, label, n_clusters, o.rep, &medoid, sh);
        if (rc) return rc;
        for (uint32_t i = 0; i < n; ++i) target[i] = sh.rep[label[i]];
        rc = mhx_dist_to(S.rows.data(), S.len.data(), n, S.stride, k, S.s(), target.data(), common.data(), denom.data(), 0);
        if (rc) return rc;
        std::string text;
        cluster_rows(S, label, sh, o.comment != 0,
                     [&](uint32_t i) {
                         const double pv = mhx_p_value(common[i], refs[i]->length, refs[target[i]]->length, k, denom[i]);
                         return fmt_g(tri_distance(common[i], denom[i], k)) + "\t" + fmt_g(pv) + "\t" + std::to_string(common[i]) + "/" + std::to_string(denom[i]);
                     },
                     text);
        if (out_msh) { rc = cluster_reps_msh(S, sh, out_msh); if (rc) return rc; }
        return put_text(text, stdout_buf, cap, need);
    });
}

// The single-linkage tree at file level: the references of all files form one set (as for the triangle), mhx_dist_mst gives
// its n - 1 merges in merge order, and the host prints them as a table or as a Newick dendrogram.
extern "C" int mhx_tree_files(const char *const *paths, int n_paths, const mhx_tree_opts *opts, char *stdout_buf, size_t cap, size_t *need)
{
    return entry("mhx_tree_files", [&]() -> int {
        mhx_tree_opts o{(uint32_t)sizeof(mhx_tree_opts), 0, 0};
        int rc = take_opts("tree", opts, o);
        if (rc) return rc;
        SetOfFiles S;
        rc = read_set_of_files("tree", paths, n_paths, S);
        if (rc) return rc;
        const std::vector<const RefSketch *> &refs = S.refs;
        const uint32_t n = S.n();
        const int k = S.k();
        const uint32_t m = n ? n - 1 : 0;
        std::vector<uint32_t> ei(m), ej(m), common(m), denom(m);
        std::vector<double> dist(m);
        rc = mhx_dist_mst(S.rows.data(), S.len.data(), n, S.stride, k, S.s(), ei.data(), ej.data(), common.data(), denom.data(), dist.data(), 0);
        if (rc) return rc;
        auto shown = [&](uint32_t i) -> const std::string & { return o.comment ? refs[i]->comment : refs[i]->name; };
        std::string text;
        if (!o.newick) { // one row per merge: the triangle's edge-list row and the clusters left after it
            for (uint32_t e = 0; e < m; ++e) {
                const double pv = mhx_p_value(common[e], refs[ei[e]]->length, refs[ej[e]]->length, k, denom[e]);
                pair_row(text, shown(ei[e]), shown(ej[e]), dist[e], pv, common[e], denom[e], std::to_string(n - 1 - e));
            }
            return put_text(text, stdout_buf, cap, need);
        }
        if (n == 0) return put_text(text, stdout_buf, cap, need);
        rc = newick_text("tree", n, ei, ej, dist, shown, text);
        if (rc) return rc;
        return put_text(text, stdout_buf, cap, need);
    });
}

// Complete / average linkage at file level: the set is read as the tree reads it, mhx_dist_linkage gives the n - 1 merges in
// merge order, and the host prints them as a table, as a Newick dendrogram, or cuts them at max_dist and prints the clusters as
// the dereplication does.
extern "C" int mhx_linkage_files(const char *const *paths, int n_paths, const mhx_linkage_opts *opts, const char *out_msh, char *stdout_buf, size_t cap,
                                 size_t *need)
{
    return entry("mhx_linkage_files", [&]() -> int {
        mhx_linkage_opts o{(uint32_t)sizeof(mhx_linkage_opts), 0, 1, 0, 0, 1.0};
        int rc = take_opts("linkage", opts, o);
        if (rc) return rc;
        if (o.linkage != 1 && o.linkage != 2) return fail(MHX_E_ARG, "linkage: linkage must be 1 (complete) or 2 (average)");
        if (o.mode < 0 || o.mode > 2) return fail(MHX_E_ARG, "linkage: mode must be 0 (merges), 1 (Newick) or 2 (cut)");
        if (o.rep != 0 && o.rep != 1) return fail(MHX_E_ARG, "linkage: rep must be 0 (first) or 1 (longest)");
        if (!(o.max_dist == o.max_dist)) return fail(MHX_E_ARG, "linkage: max_dist is not a number");
        if (out_msh && o.mode != 2) return fail(MHX_E_ARG, "linkage: an output sketch file goes with the cut (mode 2) only");
        SetOfFiles S;
        rc = read_set_of_files("linkage", paths, n_paths, S);
        if (rc) return rc;
        const std::vector<const RefSketch *> &refs = S.refs;
        const uint32_t n = S.n();
        if (out_msh) { rc = check_no_counts("linkage", refs); if (rc) return rc; }
        const uint32_t m = n ? n - 1 : 0;
        std::vector<uint32_t> ma(m), mb(m), size(m);
        std::vector<uint64_t> num(m), den(m);
        std::vector<double> dist(m);
        rc = mhx_dist_linkage(S.rows.data(), S.len.data(), n, S.stride, S.k(), S.s(), o.linkage, ma.data(), mb.data(), size.data(), num.data(), den.data(),
                              dist.data(), 0);
        if (rc) return rc;
        auto shown = [&](uint32_t i) -> const std::string & { return o.comment ? refs[i]->comment : refs[i]->name; };
        std::string text;
        if (o.mode == 0) {
            for (uint32_t e = 0; e < m; ++e)
                text += shown(ma[e]) + "\t" + shown(mb[e]) + "\t" + fmt_g(dist[e]) + "\t" + std::to_string(size[e]) + "\t" + std::to_string(n - 1 - e) + "\n";
        } else if (o.mode == 1) {
            if (n) { rc = newick_text("linkage", n, ma, mb, dist, shown, text); if (rc) return rc; }
        } else {
            std::vector<uint32_t> label(n);
            const int64_t n_clusters = mhx_linkage_labels(ma.data(), mb.data(), dist.data(), n, o.max_dist, label.data());
            if (n_clusters < 0) return (int)n_clusters;
            rc = cluster_table("linkage", S, label, (uint32_t)n_clusters, nullptr, o.comment != 0, o.rep, out_msh, text);
            if (rc) return rc;
        }
        return put_text(text, stdout_buf, cap, need);
    });
}

// Neighbour joining at file level: the set is read as the tree reads it, mhx_dist_nj gives the n - 1 joins in join order, and
// the host prints them as a table or as an UNROOTED Newick tree: every join but the last is a node "(X:len,Y:len)", the
// root is the trifurcation of the two children of join n - 3 and the node that is left, whose branch is the distance of the
// last join; children in the order of their lowest leaf (a node's id), lengths "%g" of max(0, len).
// With o.replicates = R > 0 (mhx_nj_files_opts) the joins come from mhx_dist_nj_support with their support c: the table gets a
// seventh column "c/R", and the node of every join t <= n - 4 the label floor(100 c / R) behind its ")".
static int nj_files_text(const char *const *paths, int n_paths, const mhx_nj_opts &o, char *stdout_buf, size_t cap, size_t *need)
{
    const int comment = o.comment, newick = o.newick;
    const uint32_t R = o.replicates;
    SetOfFiles S;
    int rc = read_set_of_files("nj", paths, n_paths, S);
    if (rc) return rc;
    const std::vector<const RefSketch *> &refs = S.refs;
    const uint32_t n = S.n();
    const uint32_t m = n ? n - 1 : 0;
    std::vector<uint32_t> ja(m), jb(m);
    std::vector<uint64_t> d(m), ra(m), rb(m);
    std::vector<double> la(m), lb(m);
    std::vector<uint32_t> support(R ? m : 0);
    rc = R ? mhx_dist_nj_support(S.rows.data(), S.len.data(), n, S.stride, S.k(), S.s(), R, o.keep, o.seed, ja.data(), jb.data(), d.data(), ra.data(), rb.data(),
                                 la.data(), lb.data(), support.data(), nullptr, nullptr, nullptr, 0)
           : mhx_dist_nj(S.rows.data(), S.len.data(), n, S.stride, S.k(), S.s(), ja.data(), jb.data(), d.data(), ra.data(), rb.data(), la.data(), lb.data(), 0);
    if (rc) return rc;
    auto shown = [&](uint32_t i) -> const std::string & { return comment ? refs[i]->comment : refs[i]->name; };
    auto dist = [&](uint32_t t) { return (double)d[t] * (1.0 / 4294967296.0); };
    std::string text;
    if (!newick) {
        for (uint32_t t = 0; t < m; ++t)
            text += shown(ja[t]) + "\t" + shown(jb[t]) + "\t" + fmt_g(la[t]) + "\t" + fmt_g(lb[t]) + "\t" + fmt_g(dist(t)) + "\t" + std::to_string(n - 1 - t) +
                    (R ? "\t" + std::to_string(support[t]) + "/" + std::to_string(R) : std::string()) + "\n";
        return put_text(text, stdout_buf, cap, need);
    }
    if (n == 0) return put_text(text, stdout_buf, cap, need);
    // nodes 0 .. n - 1 are the leaves, node n + t the join t; top[id]: the node that stands for the active id
    struct Node { uint32_t kid[3]; double len[3]; int kids; };
    std::vector<Node> nodes;
    std::vector<uint32_t> top(n);
    for (uint32_t i = 0; i < n; ++i) top[i] = i;
    const uint32_t binary = n >= 3 ? n - 2 : m; // joins that are nodes; the last of them takes the third child
    for (uint32_t t = 0; t < binary; ++t) {
        if (ja[t] >= n || jb[t] >= ja[t]) return fail(MHX_E_INTERNAL, "nj: join %u does not name two nodes b < a", t);
        nodes.push_back(Node{{top[jb[t]], top[ja[t]], 0}, {lb[t], la[t], 0.0}, 2});
        top[jb[t]] = n + t;
    }
    if (n >= 3) {
        Node &root = nodes.back();
        const uint32_t u = jb[n - 3], other = ja[n - 2] == u ? jb[n - 2] : ja[n - 2];
        if ((ja[n - 2] != u && jb[n - 2] != u) || other >= n || other == ja[n - 3]) return fail(MHX_E_INTERNAL, "nj: the last join does not take up the one before it");
        int at = other < jb[n - 3] ? 0 : (other < ja[n - 3] ? 1 : 2); // by lowest leaf
        for (int x = 2; x > at; --x) { root.kid[x] = root.kid[x - 1]; root.len[x] = root.len[x - 1]; }
        root.kid[at] = top[other]; root.len[at] = dist(n - 2);
        root.kids = 3;
    }
    // written without recursion: a chain of 65 535 joins is a tree of that depth
    struct Item { uint32_t node; int at; };
    std::vector<Item> todo{{nodes.empty() ? 0u : n + (uint32_t)nodes.size() - 1, 0}};
    while (!todo.empty()) {
        Item &it = todo.back();
        if (it.node < n) { text += newick_name(shown(it.node)); todo.pop_back(); continue; }
        const Node &nd = nodes[it.node - n];
        if (it.at == 0) text += "(";
        else text += ":" + fmt_g(nd.len[it.at - 1] > 0.0 ? nd.len[it.at - 1] : 0.0) + (it.at < nd.kids ? "," : ")");
        if (it.at == nd.kids) {
            const uint32_t t = it.node - n; // an inner node but the root: its support in per cent, floored
            if (R && (uint64_t)t + 4 <= n) text += std::to_string((uint64_t)100 * support[t] / R);
            todo.pop_back();
            continue;
        }
        const uint32_t kid = nd.kid[it.at++];
        todo.push_back({kid, 0});
    }
    text += ";\n";
    return put_text(text, stdout_buf, cap, need);
}

extern "C" int mhx_nj_files(const char *const *paths, int n_paths, int comment, int newick, char *stdout_buf, size_t cap, size_t *need)
{
    return entry("mhx_nj_files", [&]() -> int {
        return nj_files_text(paths, n_paths, mhx_nj_opts{(uint32_t)sizeof(mhx_nj_opts), comment, newick, 0, 0.5, 42}, stdout_buf, cap, need);
    });
}

extern "C" int mhx_nj_files_opts(const char *const *paths, int n_paths, const mhx_nj_opts *opts, char *stdout_buf, size_t cap, size_t *need)
{
    return entry("mhx_nj_files_opts", [&]() -> int {
        mhx_nj_opts o{(uint32_t)sizeof(mhx_nj_opts), 0, 0, 0, 0.5, 42};
        int rc = take_opts("nj", opts, o);
        if (rc) return rc;
        if (o.replicates) { // refused before a file is read
            if (!(o.keep > 0.0) || !(o.keep <= 1.0)) return fail(MHX_E_ARG, "nj: keep must lie in (0, 1] (%g)", o.keep);
            if (o.replicates > 10000) return fail(MHX_E_ARG, "nj: too many replicates (%u, at most 10000)", o.replicates);
        }
        return nj_files_text(paths, n_paths, o, stdout_buf, cap, need);
    });
}

namespace {

// AuriClass's clade_config.csv: a header line, then "filename,clade" split at the last comma.  clade[i] of reference i of R, whose
// name must be a filename of the table; clade_id[i] numbers the distinct clades.
int read_clades(const char *path, const SketchSet &R, std::vector<std::string> &clade, std::vector<uint32_t> &clade_id)
{
    std::vector<uint8_t> raw;
    FILE *f = fopen(path, "rb");
    if (!f) return fail(MHX_E_IO, "cannot open clade table %s", path);
    uint8_t buf[65536];
    size_t got;
    while ((got = fread(buf, 1, sizeof buf, f)) > 0) raw.insert(raw.end(), buf, buf + got);
    const bool bad = ferror(f) != 0;
    fclose(f);
    if (bad) return fail(MHX_E_IO, "cannot read clade table %s", path);
    std::unordered_map<std::string, std::string> table;
    size_t at = 0, line_no = 0;
    while (at < raw.size()) {
        size_t end = at;
        while (end < raw.size() && raw[end] != '\n') ++end;
        std::string line((const char *)raw.data() + at, end - at);
        at = end + 1;
        if (!line.empty() && line.back() == '\r') line.pop_back();
        if (line_no++ == 0 || line.empty()) continue; // the header
        const size_t comma = line.rfind(',');
        if (comma == std::string::npos) return fail(MHX_E_FORMAT, "%s: line %zu has no comma", path, line_no);
        table[line.substr(0, comma)] = line.substr(comma + 1);
    }
    std::unordered_map<std::string, uint32_t> ids;
    clade.clear();
    clade_id.clear();
    for (const RefSketch &r : R.refs) {
        const auto it = table.find(r.name);
        if (it == table.end()) return fail(MHX_E_FORMAT, "%s: no clade for reference %s", path, r.name.c_str());
        clade.push_back(it->second);
        clade_id.push_back(ids.emplace(it->second, (uint32_t)ids.size()).first->second);
    }
    return MHX_OK;
}

// Reference-set search at file level: the reference file is read, checked and staged on the device ONCE; the query files
// are read one after the other and searched in batches of sketches (mhx_dist_search's host form against the resident
// references), so that host memory holds one batch whatever n_qry is.  Rows are `mash dist` rows, per query best first.
// sup (may be null) with replicates > 0: the jackknife support of every query's hits (support_device on the rows the search
// has staged, the hits as its candidates) as a further column "c/R", and with a clade table the clade of the row's reference
// and "g/R", g the replicates whose best candidate has that clade.
int search_files_text(const char *ref_msh, const char *const *qry_msh, int n_qry, const mhx_search_opts &o, const mhx_search_support_opts *sup, uint64_t T,
                      const char *clade_csv, char *stdout_buf, size_t cap, size_t *need)
{
    const uint32_t replicates = sup ? sup->replicates : 0;
    SketchSet R;
    int rc = msh_read_file(ref_msh, R); // (checks that every hash list ascends: MHX_E_FORMAT)
    if (rc) return rc;
    std::vector<std::string> clade;
    std::vector<uint32_t> clade_id;
    if (clade_csv) { rc = read_clades(clade_csv, R, clade, clade_id); if (rc) return rc; }
    const int k = (int)R.kmer_size;
    const uint32_t nr = (uint32_t)R.refs.size();
    ResidentRefs resident;
    const SearchRefs &refs = resident.refs;
    DevArray<uint32_t> d_cand, d_ncand, d_first;
    uint32_t s = 0;
    std::string text;
    auto on_first_file = [&](const SketchSet &Q) { // the sketch size of the call, the references on the device
        s = std::max<uint32_t>(1, R.sketch_size < Q.sketch_size ? R.sketch_size : Q.sketch_size);
        return stage_refs(R, UINT32_MAX, Q.sketch_size, "the search", resident);
    };
    auto flush = [&](const std::vector<const RefSketch *> &qs) -> int {
        const uint32_t nq = (uint32_t)qs.size();
        std::vector<const uint64_t *> qrows(nq);
        std::vector<uint32_t> ql(nq), hr((size_t)nq * o.top), hc((size_t)nq * o.top), hd((size_t)nq * o.top), nh(nq), first;
        std::vector<double> hx((size_t)nq * o.top);
        for (uint32_t i = 0; i < nq; ++i) {
            qrows[i] = qs[i]->hash_data(); ql[i] = (uint32_t)qs[i]->hash_count();
            if (ql[i] > refs.stride) return fail(MHX_E_FORMAT, "query sketch %s holds more hashes than its sketch size", qs[i]->name.c_str());
        }
        SearchStaged staged{};
        const int rc2 = search_rows(qrows.data(), ql.data(), nq, refs, k, s, o.max_dist, o.top, hr.data(), hc.data(), hd.data(), hx.data(), nh.data(), &staged);
        if (rc2) return rc2;
        if (replicates) { // the hits, before the p-value drops rows, are the candidates; the queries are on the device still
            const size_t cells = (size_t)nq * o.top;
            if (d_cand.grow(cells) != hipSuccess || d_first.grow(cells) != hipSuccess || d_ncand.grow(nq) != hipSuccess)
                return fail(MHX_E_HIP, "hipMalloc failed for the candidates of the support");
            if (hipMemcpy(d_cand, hr.data(), cells * 4, hipMemcpyHostToDevice) != hipSuccess || hipMemcpy(d_ncand, nh.data(), (size_t)nq * 4, hipMemcpyHostToDevice) != hipSuccess)
                return fail(MHX_E_HIP, "H2D copy of the candidates failed");
            SupportCall c{};
            c.q = staged.q; c.q_len = staged.q_len; c.r = refs.rows; c.r_len = refs.len; c.nq = nq; c.nr = nr; c.stride = refs.stride; c.s = s;
            c.cand = d_cand; c.n_cand = d_ncand; c.top = o.top; c.replicates = replicates; c.keep = sup->keep; c.seed = sup->seed; c.T = T;
            c.first = d_first;
            const int rc3 = support_device(c);
            if (rc3) return rc3;
            first.resize(cells);
            if (hipMemcpy(first.data(), d_first, cells * 4, hipMemcpyDeviceToHost) != hipSuccess) return fail(MHX_E_HIP, "D2H copy of the support failed");
        }
        const std::string of = "/" + std::to_string(replicates);
        for (uint32_t qi = 0; qi < nq; ++qi)
            for (uint32_t t = 0; t < nh[qi]; ++t) {
                const size_t p = (size_t)qi * o.top + t;
                const RefSketch &ref = R.refs[hr[p]];
                const double pv = mhx_p_value(hc[p], ref.length, qs[qi]->length, k, hd[p]);
                if (!(pv <= o.max_p_value)) continue; // drops a row, never promotes a lower-ranked pair
                std::string more;
                if (replicates) {
                    more = std::to_string(first[p]) + of;
                    if (clade_csv) {
                        uint32_t same = 0; // replicates whose best candidate has this row's clade
                        for (uint32_t x = 0; x < nh[qi]; ++x)
                            if (clade_id[hr[(size_t)qi * o.top + x]] == clade_id[hr[p]]) same += first[(size_t)qi * o.top + x];
                        more += "\t" + clade[hr[p]] + "\t" + std::to_string(same) + of;
                    }
                }
                pair_row(text, ref.name, qs[qi]->name, hx[p], pv, hc[p], hd[p], more);
            }
        return MHX_OK;
    };
    rc = walk_query_files(R, qry_msh, n_qry, on_first_file, flush);
    if (rc) return rc;
    return put_text(text, stdout_buf, cap, need);
}

int search_files_check(const char *cmd, const char *ref_msh, const char *const *qry_msh, int n_qry, const mhx_search_opts &o)
{
    const int rc = set_paths_check(cmd, ref_msh, qry_msh, n_qry);
    if (rc) return rc;
    if (o.top < 1 || o.top > 64) return fail(MHX_E_ARG, "%s: top must be 1 .. 64", cmd);
    if (!(o.max_dist == o.max_dist) || !(o.max_p_value == o.max_p_value)) return fail(MHX_E_ARG, "%s: max_dist / max_p_value is not a number", cmd);
    return MHX_OK;
}

} // namespace

extern "C" int mhx_search_files(const char *ref_msh, const char *const *qry_msh, int n_qry, const mhx_search_opts *opts, char *stdout_buf, size_t cap, size_t *need)
{
    return entry("mhx_search_files", [&]() -> int {
        mhx_search_opts o{(uint32_t)sizeof(mhx_search_opts), 5, 1.0, 1.0};
        int rc = ref_msh && qry_msh && n_qry >= 1 ? take_opts("search", opts, o) : MHX_OK;
        if (rc == MHX_OK) rc = search_files_check("search", ref_msh, qry_msh, n_qry, o);
        if (rc) return rc;
        return search_files_text(ref_msh, qry_msh, n_qry, o, nullptr, 0, nullptr, stdout_buf, cap, need);
    });
}

// `mash dist -d D -v P REF QUERY [QUERY ...]`: every reference within D of every query sketch.  The reference file is read,
// checked and staged on the device once, as the search does; the query files are read one after the other and go to
// within_rows in batches of sketches, whose CSR the host prints row by row -- in reference order, or every row of the CSR
// sorted best first by search_better.  A batch whose hits exceed its buffers is repeated once with the size it reported.
extern "C" int mhx_within_files(const char *ref_msh, const char *const *qry_msh, int n_qry, const mhx_within_opts *opts, char *stdout_buf, size_t cap, size_t *need)
{
    return entry("mhx_within_files", [&]() -> int {
        mhx_within_opts o{(uint32_t)sizeof(mhx_within_opts), 0, 1.0, 1.0};
        int rc = set_paths_check("within", ref_msh, qry_msh, n_qry);
        if (rc == MHX_OK) rc = take_opts("within", opts, o);
        if (rc) return rc;
        if (o.order > 1) return fail(MHX_E_ARG, "within: order must be 0 (reference order) or 1 (best first)");
        if (!(o.max_dist == o.max_dist) || !(o.max_p_value == o.max_p_value)) return fail(MHX_E_ARG, "within: max_dist / max_p_value is not a number");
        SketchSet R;
        rc = msh_read_file(ref_msh, R); // (checks that every hash list ascends: MHX_E_FORMAT)
        if (rc) return rc;
        const int k = (int)R.kmer_size;
        const uint32_t nr = (uint32_t)R.refs.size();
        ResidentRefs resident;
        const SearchRefs &refs = resident.refs;
        uint32_t s = 0;
        std::string text;
        constexpr uint64_t kFirstRoom = 4096; // hits the buffers hold before a batch has asked for more
        std::vector<uint32_t> hr, hc, hd, order;
        std::vector<double> hx;
        auto on_first_file = [&](const SketchSet &Q) { // the sketch size of the call, the references on the device
            s = std::max<uint32_t>(1, R.sketch_size < Q.sketch_size ? R.sketch_size : Q.sketch_size);
            return stage_refs(R, UINT32_MAX, Q.sketch_size, "within", resident);
        };
        auto flush = [&](const std::vector<const RefSketch *> &qs) -> int {
            const uint32_t nq = (uint32_t)qs.size();
            std::vector<const uint64_t *> qrows(nq);
            std::vector<uint32_t> ql(nq);
            std::vector<uint64_t> row_off((size_t)nq + 1);
            for (uint32_t i = 0; i < nq; ++i) {
                qrows[i] = qs[i]->hash_data(); ql[i] = (uint32_t)qs[i]->hash_count();
                if (ql[i] > refs.stride) return fail(MHX_E_FORMAT, "query sketch %s holds more hashes than its sketch size", qs[i]->name.c_str());
            }
            uint64_t found = 0, room = std::max<uint64_t>(hr.size(), std::min<uint64_t>((uint64_t)nq * nr, kFirstRoom));
            int rc2 = MHX_OK;
            for (int attempt = 0; attempt < 2; ++attempt) {
                if (hr.size() < room) { hr.resize(room); hc.resize(room); hd.resize(room); hx.resize(room); }
                rc2 = within_rows(qrows.data(), ql.data(), nq, refs, k, s, o.max_dist, row_off.data(), hr.data(), hc.data(), hd.data(), hx.data(), hr.size(), &found);
                if (rc2 != MHX_E_CAPACITY) break;
                room = found;
            }
            if (rc2) return rc2;
            clear_error();
            for (uint32_t qi = 0; qi < nq; ++qi) {
                const uint64_t lo = row_off[qi], hi = row_off[qi + 1];
                order.resize((size_t)(hi - lo));
                for (uint64_t t = lo; t < hi; ++t) order[(size_t)(t - lo)] = (uint32_t)(t - lo);
                if (o.order == 1)
                    std::sort(order.begin(), order.end(), [&](uint32_t a, uint32_t b) {
                        return search_better(SearchHit{hr[lo + a], hc[lo + a], hd[lo + a]}, SearchHit{hr[lo + b], hc[lo + b], hd[lo + b]});
                    });
                for (const uint32_t t : order) {
                    const size_t p = (size_t)(lo + t);
                    const RefSketch &ref = R.refs[hr[p]];
                    const double pv = mhx_p_value(hc[p], ref.length, qs[qi]->length, k, hd[p]);
                    if (!(pv <= o.max_p_value)) continue;
                    pair_row(text, ref.name, qs[qi]->name, hx[p], pv, hc[p], hd[p]);
                }
            }
            return MHX_OK;
        };
        rc = walk_query_files(R, qry_msh, n_qry, on_first_file, flush);
        if (rc) return rc;
        return put_text(text, stdout_buf, cap, need);
    });
}

// The search with the jackknife support of its hits.  replicates == 0: exactly mhx_search_files.
extern "C" int mhx_search_files_support(const char *ref_msh, const char *const *qry_msh, int n_qry, const mhx_search_support_opts *opts, const char *clade_csv,
                                        char *stdout_buf, size_t cap, size_t *need)
{
    return entry("mhx_search_files_support", [&]() -> int {
        mhx_search_support_opts so{(uint32_t)sizeof(mhx_search_support_opts), 5, 1.0, 1.0, 0, 0.5, 42};
        int rc = ref_msh && qry_msh && n_qry >= 1 ? take_opts("search_support", opts, so) : MHX_OK;
        const mhx_search_opts o{(uint32_t)sizeof(mhx_search_opts), so.top, so.max_dist, so.max_p_value};
        if (rc == MHX_OK) rc = search_files_check("search", ref_msh, qry_msh, n_qry, o);
        if (rc) return rc;
        uint64_t T = 0;
        if (so.replicates == 0) {
            if (clade_csv) return fail(MHX_E_ARG, "search: a clade table needs replicates");
            return search_files_text(ref_msh, qry_msh, n_qry, o, nullptr, 0, nullptr, stdout_buf, cap, need);
        }
        rc = support_check(1, 1, so.top, so.replicates, so.keep, &T); // refused before a file is read
        if (rc) return rc;
        return search_files_text(ref_msh, qry_msh, n_qry, o, &so, T, clade_csv, stdout_buf, cap, need);
    });
}

// Containment at file level: the reference file is read and checked once; the query files are read one after the other and
// go to the device in batches of sketches (contain_rows, every list from where it lies), so that host memory holds one
// batch whatever n_qry is.  The two sketch sizes stay apart: every set is cut at its own.
// winner: the winner-take-all passes run behind the plain one, the genome lengths of the reference file ranking ties, and what a
// reference won stands in the place of what it shares -- in identity, p-value, both fractions and the filters.
static int contain_files_text(const char *ref_msh, const char *const *qry_msh, int n_qry, const mhx_contain_opts *opts, bool winner, char *stdout_buf, size_t cap,
                              size_t *need)
{
    mhx_contain_opts o{(uint32_t)sizeof(mhx_contain_opts), 0, 0.0, 1.0};
    int rc = ref_msh && qry_msh && n_qry >= 1 ? take_opts("contain", opts, o) : MHX_OK;
    if (rc) return rc;
    rc = set_paths_check("contain", ref_msh, qry_msh, n_qry);
    if (rc) return rc;
    if (!(o.min_identity == o.min_identity) || !(o.max_p_value == o.max_p_value)) return fail(MHX_E_ARG, "contain: min_identity / max_p_value is not a number");
    SketchSet R;
    rc = msh_read_file(ref_msh, R); // (checks that every hash list ascends: MHX_E_FORMAT)
    if (rc) return rc;
    const int k = (int)R.kmer_size;
    const uint32_t nr = (uint32_t)R.refs.size(), s_r = std::max<uint32_t>(1, R.sketch_size);
    std::vector<const uint64_t *> rrows(nr);
    std::vector<uint32_t> rl(nr);
    std::vector<uint64_t> r_length(nr);
    uint32_t r_longest = 0;
    for (uint32_t i = 0; i < nr; ++i) {
        rrows[i] = R.refs[i].hash_data(); rl[i] = (uint32_t)R.refs[i].hash_count(); r_length[i] = R.refs[i].length;
        r_longest = std::max(r_longest, rl[i]);
    }
    uint32_t q_sketch_size = 0;
    std::string text;
    auto on_first_file = [&](const SketchSet &Q) { q_sketch_size = Q.sketch_size; return MHX_OK; };
    auto flush = [&](const std::vector<const RefSketch *> &qs) -> int {
        const uint32_t nq = (uint32_t)qs.size();
        std::vector<const uint64_t *> qrows(nq);
        std::vector<uint32_t> ql(nq);
        uint32_t longest = r_longest;
        for (uint32_t i = 0; i < nq; ++i) {
            qrows[i] = qs[i]->hash_data(); ql[i] = (uint32_t)qs[i]->hash_count();
            longest = std::max(longest, ql[i]);
        }
        const size_t cells = (size_t)nq * nr;
        std::vector<uint32_t> shared(cells), n_q(cells), n_r(cells), won(winner ? cells : 0);
        const int rc2 = contain_rows(qrows.data(), nullptr, ql.data(), nq, std::max<uint32_t>(1, q_sketch_size), rrows.data(), nullptr, rl.data(), nr, s_r,
                                     row_stride(longest), shared.data(), n_q.data(), n_r.data(), winner ? r_length.data() : nullptr, winner ? won.data() : nullptr);
        if (rc2) return rc2;
        if (winner) shared.swap(won); // the rows below print what was won
        for (uint32_t qi = 0; qi < nq; ++qi)
            for (uint32_t ri = 0; ri < nr; ++ri) {
                const size_t p = (size_t)qi * nr + ri;
                const double identity = n_r[p] == 0 ? 0.0 : mhx_screen_identity(shared[p], n_r[p], k);
                const double pv = n_r[p] == 0 ? 1.0 : mhx_screen_p_value(shared[p], n_r[p], (double)qs[qi]->length, k);
                if (!(identity >= o.min_identity) || !(pv <= o.max_p_value)) continue;
                text += (o.comment ? R.refs[ri].comment : R.refs[ri].name) + "\t" + (o.comment ? qs[qi]->comment : qs[qi]->name) + "\t" + fmt_g(identity) +
                        "\t" + fmt_g(pv) + "\t" + std::to_string(shared[p]) + "/" + std::to_string(n_r[p]) + "\t" + std::to_string(shared[p]) + "/" +
                        std::to_string(n_q[p]) + "\n";
            }
        return MHX_OK;
    };
    rc = walk_query_files(R, qry_msh, n_qry, on_first_file, flush);
    if (rc) return rc;
    return put_text(text, stdout_buf, cap, need);
}

extern "C" int mhx_contain_files(const char *ref_msh, const char *const *qry_msh, int n_qry, const mhx_contain_opts *opts, char *stdout_buf, size_t cap, size_t *need)
{
    return entry("mhx_contain_files", [&]() -> int { return contain_files_text(ref_msh, qry_msh, n_qry, opts, false, stdout_buf, cap, need); });
}

extern "C" int mhx_contain_files_winner(const char *ref_msh, const char *const *qry_msh, int n_qry, const mhx_contain_opts *opts, char *stdout_buf, size_t cap,
                                        size_t *need)
{
    return entry("mhx_contain_files_winner", [&]() -> int { return contain_files_text(ref_msh, qry_msh, n_qry, opts, true, stdout_buf, cap, need); });
}

// Containment search at file level: the reference file is read, checked and staged on the device ONCE, every list cut at the
// reference sketch size; the query files are read one after the other and searched in batches of sketches
// (contain_search_rows against the resident references), so that host memory holds one batch and at most top rows per query
// whatever n_qry and the size of the reference set are.  Rows are mhx_contain_files's, per query best first.
extern "C" int mhx_contain_files_search(const char *ref_msh, const char *const *qry_msh, int n_qry, const mhx_contain_search_opts *opts, char *stdout_buf,
                                        size_t cap, size_t *need)
{
    return entry("mhx_contain_files_search", [&]() -> int {
        mhx_contain_search_opts o{(uint32_t)sizeof(mhx_contain_search_opts), 0, 5, 1, 0.0, 1.0};
        int rc = ref_msh && qry_msh && n_qry >= 1 ? take_opts("contain_search", opts, o) : MHX_OK;
        if (rc) return rc;
        rc = set_paths_check("contain", ref_msh, qry_msh, n_qry);
        if (rc) return rc;
        if (!(o.min_identity == o.min_identity) || !(o.max_p_value == o.max_p_value)) return fail(MHX_E_ARG, "contain: min_identity / max_p_value is not a number");
        if (o.top < 1 || o.top > 64) return fail(MHX_E_ARG, "contain: top must be 1 .. 64");
        if (o.min_shared < 1) return fail(MHX_E_ARG, "contain: min_shared must be at least 1");
        SketchSet R;
        rc = msh_read_file(ref_msh, R); // (checks that every hash list ascends: MHX_E_FORMAT)
        if (rc) return rc;
        const int k = (int)R.kmer_size;
        const uint32_t s_r = std::max<uint32_t>(1, R.sketch_size);
        ResidentRefs resident;
        const SearchRefs &refs = resident.refs;
        uint32_t s_q = 1;
        std::string text;
        auto on_first_file = [&](const SketchSet &Q) { // the queries' sketch size, the references on the device, cut at theirs
            s_q = std::max<uint32_t>(1, Q.sketch_size);
            return stage_refs(R, s_r, s_q, "the containment search", resident);
        };
        auto flush = [&](const std::vector<const RefSketch *> &qs) -> int {
            const uint32_t nq = (uint32_t)qs.size();
            std::vector<const uint64_t *> qrows(nq);
            std::vector<uint32_t> ql(nq), hr((size_t)nq * o.top), hs((size_t)nq * o.top), hnr((size_t)nq * o.top), hnq((size_t)nq * o.top), nh(nq);
            for (uint32_t i = 0; i < nq; ++i) { // a list is the first s_q entries of its sketch at most
                qrows[i] = qs[i]->hash_data(); ql[i] = (uint32_t)std::min<size_t>(qs[i]->hash_count(), s_q);
            }
            const int rc2 = contain_search_rows(qrows.data(), ql.data(), nq, s_q, refs, s_r, k, o.min_identity, o.min_shared, o.top, hr.data(), hs.data(),
                                                hnr.data(), hnq.data(), nh.data());
            if (rc2) return rc2;
            for (uint32_t qi = 0; qi < nq; ++qi)
                for (uint32_t t = 0; t < nh[qi]; ++t) {
                    const size_t p = (size_t)qi * o.top + t;
                    const RefSketch &ref = R.refs[hr[p]];
                    const double identity = mhx_screen_identity(hs[p], hnr[p], k);
                    const double pv = mhx_screen_p_value(hs[p], hnr[p], (double)qs[qi]->length, k);
                    if (!(pv <= o.max_p_value)) continue; // drops a row, never promotes a lower-ranked pair
                    text += (o.comment ? ref.comment : ref.name) + "\t" + (o.comment ? qs[qi]->comment : qs[qi]->name) + "\t" + fmt_g(identity) + "\t" +
                            fmt_g(pv) + "\t" + std::to_string(hs[p]) + "/" + std::to_string(hnr[p]) + "\t" + std::to_string(hs[p]) + "/" +
                            std::to_string(hnq[p]) + "\n";
                }
            return MHX_OK;
        };
        rc = walk_query_files(R, qry_msh, n_qry, on_first_file, flush);
        if (rc) return rc;
        return put_text(text, stdout_buf, cap, need);
    });
}

// Every reference a query holds, at file level: the reference file is read, checked and staged on the device ONCE, as
// mhx_contain_files_search does; the query files are read one after the other and go to contain_within_rows in batches of
// sketches, whose CSR the host prints row by row -- in reference order, or every row of the CSR sorted best first by
// contain_better.  A batch whose hits exceed its buffers is repeated once with the size it reported.
extern "C" int mhx_contain_files_within(const char *ref_msh, const char *const *qry_msh, int n_qry, const mhx_contain_within_opts *opts, char *stdout_buf,
                                        size_t cap, size_t *need)
{
    return entry("mhx_contain_files_within", [&]() -> int {
        mhx_contain_within_opts o{(uint32_t)sizeof(mhx_contain_within_opts), 0, 1, 0.0, 1, 1.0};
        int rc = ref_msh && qry_msh && n_qry >= 1 ? take_opts("contain_within", opts, o) : MHX_OK;
        if (rc) return rc;
        rc = set_paths_check("contain", ref_msh, qry_msh, n_qry);
        if (rc) return rc;
        if (!(o.min_identity == o.min_identity) || !(o.max_p_value == o.max_p_value)) return fail(MHX_E_ARG, "contain: min_identity / max_p_value is not a number");
        if (o.order > 1) return fail(MHX_E_ARG, "contain: order must be 0 (reference order) or 1 (best first)");
        if (o.min_shared < 1) return fail(MHX_E_ARG, "contain: min_shared must be at least 1");
        SketchSet R;
        rc = msh_read_file(ref_msh, R); // (checks that every hash list ascends: MHX_E_FORMAT)
        if (rc) return rc;
        const int k = (int)R.kmer_size;
        const uint32_t nr = (uint32_t)R.refs.size(), s_r = std::max<uint32_t>(1, R.sketch_size);
        ResidentRefs resident;
        const SearchRefs &refs = resident.refs;
        uint32_t s_q = 1;
        std::string text;
        constexpr uint64_t kFirstRoom = 4096; // hits the buffers hold before a batch has asked for more
        std::vector<uint32_t> hr, hs, hnr, hnq, order;
        auto on_first_file = [&](const SketchSet &Q) { // the queries' sketch size, the references on the device, cut at theirs
            s_q = std::max<uint32_t>(1, Q.sketch_size);
            return stage_refs(R, s_r, s_q, "contain --all", resident);
        };
        auto flush = [&](const std::vector<const RefSketch *> &qs) -> int {
            const uint32_t nq = (uint32_t)qs.size();
            std::vector<const uint64_t *> qrows(nq);
            std::vector<uint32_t> ql(nq);
            std::vector<uint64_t> row_off((size_t)nq + 1);
            for (uint32_t i = 0; i < nq; ++i) { // a list is the first s_q entries of its sketch at most
                qrows[i] = qs[i]->hash_data(); ql[i] = (uint32_t)std::min<size_t>(qs[i]->hash_count(), s_q);
            }
            uint64_t found = 0, room = std::max<uint64_t>(hr.size(), std::min<uint64_t>((uint64_t)nq * nr, kFirstRoom));
            int rc2 = MHX_OK;
            for (int attempt = 0; attempt < 2; ++attempt) {
                if (hr.size() < room) { hr.resize(room); hs.resize(room); hnr.resize(room); hnq.resize(room); }
                rc2 = contain_within_rows(qrows.data(), ql.data(), nq, s_q, refs, s_r, k, o.min_identity, o.min_shared, row_off.data(), hr.data(), hs.data(),
                                          hnr.data(), hnq.data(), hr.size(), &found);
                if (rc2 != MHX_E_CAPACITY) break;
                room = found;
            }
            if (rc2) return rc2;
            clear_error();
            for (uint32_t qi = 0; qi < nq; ++qi) {
                const uint64_t lo = row_off[qi], hi = row_off[qi + 1];
                order.resize((size_t)(hi - lo));
                for (uint64_t t = lo; t < hi; ++t) order[(size_t)(t - lo)] = (uint32_t)(t - lo);
                if (o.order == 1)
                    std::sort(order.begin(), order.end(), [&](uint32_t a, uint32_t b) {
                        return contain_better(ContainHit{hr[lo + a], hs[lo + a], hnr[lo + a], hnq[lo + a]}, ContainHit{hr[lo + b], hs[lo + b], hnr[lo + b], hnq[lo + b]});
                    });
                for (const uint32_t t : order) {
                    const size_t p = (size_t)(lo + t);
                    const RefSketch &ref = R.refs[hr[p]];
                    const double identity = mhx_screen_identity(hs[p], hnr[p], k);
                    const double pv = mhx_screen_p_value(hs[p], hnr[p], (double)qs[qi]->length, k);
                    if (!(pv <= o.max_p_value)) continue;
                    text += (o.comment ? ref.comment : ref.name) + "\t" + (o.comment ? qs[qi]->comment : qs[qi]->name) + "\t" + fmt_g(identity) + "\t" +
                            fmt_g(pv) + "\t" + std::to_string(hs[p]) + "/" + std::to_string(hnr[p]) + "\t" + std::to_string(hs[p]) + "/" +
                            std::to_string(hnq[p]) + "\n";
                }
            }
            return MHX_OK;
        };
        rc = walk_query_files(R, qry_msh, n_qry, on_first_file, flush);
        if (rc) return rc;
        return put_text(text, stdout_buf, cap, need);
    });
}
