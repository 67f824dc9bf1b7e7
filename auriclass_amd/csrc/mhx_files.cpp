// mhx_files.cpp -- the file-level half of libmhx: FASTQ / FASTA ingest (bulk path for uncompressed
// files, inflate threads for .gz, whole-file record parser as the last resort) and the calls that read
// sequence files (mhx_sketch_files*, mhx_screen_files*).  The commands over sketch sets, `mash dist` first, are in
// mhx_files_sets.cpp; together they replace AuriClass's `mash sketch` / `mash dist` subprocesses
// (/root/reference/auriclass/classes.py:576-596, 696-713, 92-104).
#include <hip/hip_runtime.h>
#include <fcntl.h>
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <sys/mman.h>
#include <sys/stat.h>
#include <unistd.h>

#include <zlib.h>
#if defined(__x86_64__)
#include <immintrin.h>
#endif

#include <algorithm>
#include <chrono>
#include <condition_variable>
#include <deque>
#include <exception>
#include <memory>
#include <mutex>
#include <new>
#include <string>
#include <thread>
#include <vector>

#include "mhx_device.h"
#include "mhx_engine_internal.h"
#include "mhx_internal.h"

using namespace mhx;

// ---- file level -------------------------------------------------------------------------
namespace mhx {
int put_text(const std::string &t, char *buf, size_t cap, size_t *need)
{
    if (need) *need = t.size() + 1;
    if (cap == 0) return MHX_OK;
    if (!buf || cap < t.size() + 1) return fail(MHX_E_CAPACITY, "text buffer too small (%zu needed)", t.size() + 1);
    memcpy(buf, t.c_str(), t.size() + 1);
    return MHX_OK;
}
} // namespace mhx

static std::string make_comment(const std::string &name, const std::string &comment, uint64_t count)
{ // mash sketchFile(): "<name> <comment>", wrapped when several records were counted
    std::string c = name + " " + comment;
    if (count > 1) c = "[" + std::to_string(count) + " seqs] " + c + " [...]";
    return c;
}

struct Loaded {
    std::vector<uint8_t> raw;  // inflated file
    ParsedRecords rec;         // filled when the record parser path is used
    bool fastq4 = false;
};

// `mash screen` at file level: the prober of `scr` rides along with the sketcher the ingest is about to feed (every span
// reaches both), starting from zero counts -- an attempt that was given up leaves nothing behind.
static int attach_screen(mhx_sketcher *sk, mhx_screener *scr)
{
    if (!scr || !sk) return MHX_OK;
    const int rc = mhx_screener_reset(scr);
    if (rc) return rc;
    sketcher_set_follower(sk, screener_prober(scr));
    return MHX_OK;
}

// One reference from one or more inputs on the device.  On a 4-line violation or a too
// tight admission bound the whole reference is redone (record parser / bigger table).
static int sketch_reference(const std::vector<Loaded *> &inputs, int k, uint32_t s, uint32_t m, bool allow_device_fastq,
                            std::vector<uint64_t> &hashes, std::vector<uint32_t> &counts, uint64_t *kmers, mhx_screener *scr = nullptr)
{
    uint64_t total = 0;
    for (auto *in : inputs) total += in->raw.size();
    bool device_fastq = allow_device_fastq;
    uint64_t boost = 1;
    for (int attempt = 0; attempt < 6; ++attempt) {
        mhx_sketcher *sk = nullptr;
        int rc = create_sketcher(k, s, m, total, boost, &sk);
        if (rc) return rc;
        sketcher_verify_fastq(sk, true); // a whole-file FASTQ4 push starts at the file's first record
        rc = attach_screen(sk, scr);
        if (rc) { mhx_sketcher_destroy(sk); return rc; }
        for (auto *in : inputs) {
            if (device_fastq && in->fastq4) {
                rc = mhx_sketcher_push_host(sk, in->raw.data(), in->raw.size(), MHX_FMT_FASTQ4);
            } else {
                if (in->rec.records_seen == 0 && in->rec.seq.empty()) {
                    if (allow_device_fastq) g.last_fastq_route = MHX_ROUTE_RECORD_PARSER; // (a reads call: mhx_last_fastq_route)
                    rc = parse_fastx(in->raw.data(), in->raw.size(), k, in->rec);
                    if (rc) { mhx_sketcher_destroy(sk); return rc; } // the record parser's verdict is final (not the device parser's MHX_E_FORMAT, which sends the file HERE)
                }
                rc = mhx_sketcher_push_host(sk, in->rec.seq.data(), in->rec.seq.size(), MHX_FMT_SEQ);
            }
            if (rc) break;
        }
        uint32_t n = 0;
        if (!rc) {
            hashes.resize(s);
            counts.resize(s);
            rc = mhx_sketcher_finish(sk, hashes.data(), counts.data(), &n);
        }
        if (!rc && kmers) {
            uint64_t st[8];
            rc = mhx_sketcher_stats(sk, st);
            *kmers = st[0];
        }
        mhx_sketcher_destroy(sk);
        if (rc == MHX_E_FORMAT && device_fastq) { device_fastq = false; continue; }
        if (rc == MHX_E_CAPACITY) { boost *= 16; continue; }
        if (rc) return rc;
        hashes.resize(n);
        counts.resize(n);
        return MHX_OK;
    }
    return fail(MHX_E_CAPACITY, "could not size the device table for this input");
}

// ---- streaming FASTQ ingest ---------------------------------------------------------------
// Reads mode on real inputs is inflate-bound (zlib, ~0.1-0.3 GB/s per stream), so every input
// file gets its own inflate thread; each thread cuts its stream into <= 32 MiB chunks at record
// boundaries (a multiple of four lines since the start of the file) and hands them to the
// caller's thread, which copies them to the device and pushes them through the FASTQ kernel
// while the other files keep inflating.  Host memory stays bounded (a few chunks per file).
namespace {
constexpr size_t kIngestChunk = 32u << 20;

// Host buffers of the chunk pipeline.  Pinned (hipHostMalloc) when possible: the copy to the device then runs at the
// link's rate on the copy stream while the host thread goes on, instead of being staged through the runtime's bounce
// buffer.  Pinning 32 MiB costs milliseconds, so the engine keeps the buffers between calls (Engine::ingest_pinned);
// at most `limit` are in use per call, producers wait for one to come back.
struct HostBuf {
    uint8_t *p = nullptr;
    bool pinned = false;
};

class BufPool {
  public:
    BufPool(size_t bytes, size_t limit) : bytes_(bytes), limit_(limit) {}
    ~BufPool()
    {
        for (auto &b : spare_) {
            if (b.pinned && g.ready && g.ingest_pinned.size() < Engine::kIngestPinnedKeep) g.ingest_pinned.emplace_back(b.p, bytes_);
            else if (b.pinned) hipHostFree(b.p);
            else free(b.p);
        }
    }
    HostBuf take()
    {
        std::unique_lock<std::mutex> lk(m_);
        for (;;) {
            if (!spare_.empty()) { HostBuf b = spare_.back(); spare_.pop_back(); return b; }
            if (allocated_ < limit_ || abort_) break; // (after an abort nobody gives buffers back: let the producer run out)
            cv_.wait(lk);
        }
        ++allocated_;
        if (!g.ingest_pinned.empty()) { HostBuf b{g.ingest_pinned.back().release(), true}; g.ingest_pinned.pop_back(); return b; }
        lk.unlock();
        HostBuf b;
        static const bool no_pin = getenv("MHX_INGEST_PAGEABLE") != nullptr;
        (void)hipSetDevice(g.device); // producers are threads of their own
        if (!no_pin && hipHostMalloc((void **)&b.p, bytes_, hipHostMallocDefault) == hipSuccess) b.pinned = true;
        else { (void)hipGetLastError(); b.p = (uint8_t *)malloc(bytes_); b.pinned = false; }
        if (!b.p) throw std::bad_alloc();
        return b;
    }
    void give(HostBuf b)
    {
        if (!b.p) return;
        { std::lock_guard<std::mutex> lk(m_); spare_.push_back(b); }
        cv_.notify_one();
    }
    void abort() { { std::lock_guard<std::mutex> lk(m_); abort_ = true; } cv_.notify_all(); }

  private:
    std::mutex m_;
    std::condition_variable cv_;
    std::vector<HostBuf> spare_;
    size_t bytes_, limit_, allocated_ = 0;
    bool abort_ = false;
};

// One record-aligned piece of an inflated FASTQ.  The buffer keeps GzInflater::kWindow bytes of room in
// front of the data: the previous 32 KiB of the stream, which DEFLATE matches may still refer to.
struct IngestChunk {
    HostBuf buf;           // kWindow + kIngestChunk + slack bytes, not zero-filled; goes back to `pool` with the chunk
    BufPool *pool = nullptr;
    size_t size = 0;
    int file = 0;
    bool first_of_file = false;
    IngestChunk() = default;
    IngestChunk(const IngestChunk &) = delete;
    IngestChunk &operator=(const IngestChunk &) = delete;
    IngestChunk(IngestChunk &&o) noexcept { *this = std::move(o); }
    IngestChunk &operator=(IngestChunk &&o) noexcept
    {
        if (this != &o) {
            release();
            buf = o.buf; pool = o.pool; size = o.size; file = o.file; first_of_file = o.first_of_file;
            o.buf = HostBuf(); o.pool = nullptr;
        }
        return *this;
    }
    ~IngestChunk() { release(); }
    void release() { if (pool && buf.p) pool->give(buf); buf = HostBuf(); }
    uint8_t *data() { return buf.p + GzInflater::kWindow; }
    static size_t alloc_bytes() { return GzInflater::kWindow + kIngestChunk + GzInflater::kOvershoot + 64; }
};

class ChunkQueue {
  public:
    void put(IngestChunk &&c)
    {
        std::unique_lock<std::mutex> lk(m_);
        room_.wait(lk, [&] { return q_.size() < 4 || abort_; });
        if (abort_) return;
        q_.push_back(std::move(c));
        ready_.notify_one();
    }
    bool get(IngestChunk &out) // false when every producer is done and the queue is empty
    {
        std::unique_lock<std::mutex> lk(m_);
        ready_.wait(lk, [&] { return !q_.empty() || live_ == 0; });
        if (q_.empty()) return false;
        out = std::move(q_.front());
        q_.pop_front();
        room_.notify_one();
        return true;
    }
    // chunk buffers go round (BufPool): fresh 32 MiB allocations cost more in page faults than the inflate that fills them
    explicit ChunkQueue(size_t max_buffers) : pool_(IngestChunk::alloc_bytes(), max_buffers) {}
    void take_buffer(IngestChunk &c) { c.release(); c.buf = pool_.take(); c.pool = &pool_; }
    void producer_started() { std::lock_guard<std::mutex> lk(m_); ++live_; }
    void producer_done() { std::lock_guard<std::mutex> lk(m_); --live_; ready_.notify_all(); }
    void abort() { { std::lock_guard<std::mutex> lk(m_); abort_ = true; room_.notify_all(); } pool_.abort(); }
    bool aborted() { std::lock_guard<std::mutex> lk(m_); return abort_; }

  private:
    std::mutex m_;
    std::condition_variable ready_, room_;
    BufPool pool_; // before q_: chunks still queued (after an abort) hand their buffers back to it
    std::deque<IngestChunk> q_;
    int live_ = 0;
    bool abort_ = false;
};

struct FileIngestState {
    std::string error;
    uint64_t lines = 0, bytes = 0;
    bool not_fastq4 = false;
    bool own_inflate_failed = false; // the engine's own DEFLATE decoder refused the stream
};

static bool is_gzip_file(const char *path)
{
    FILE *f = fopen(path, "rb");
    uint8_t magic[2] = {0, 0};
    if (f) { if (fread(magic, 1, 2, f) != 2) magic[0] = 0; fclose(f); }
    return magic[0] == 0x1f && magic[1] == 0x8b;
}

#if defined(__x86_64__)
__attribute__((target("avx2,popcnt"))) static size_t count_newlines_avx2(const uint8_t *p, size_t n)
{
    const __m256i nl = _mm256_set1_epi8('\n');
    size_t c = 0, i = 0;
    for (; i + 128 <= n; i += 128) {
        const uint32_t m0 = (uint32_t)_mm256_movemask_epi8(_mm256_cmpeq_epi8(_mm256_loadu_si256((const __m256i *)(p + i)), nl));
        const uint32_t m1 = (uint32_t)_mm256_movemask_epi8(_mm256_cmpeq_epi8(_mm256_loadu_si256((const __m256i *)(p + i + 32)), nl));
        const uint32_t m2 = (uint32_t)_mm256_movemask_epi8(_mm256_cmpeq_epi8(_mm256_loadu_si256((const __m256i *)(p + i + 64)), nl));
        const uint32_t m3 = (uint32_t)_mm256_movemask_epi8(_mm256_cmpeq_epi8(_mm256_loadu_si256((const __m256i *)(p + i + 96)), nl));
        c += (size_t)__builtin_popcountll(((uint64_t)m1 << 32) | m0) + (size_t)__builtin_popcountll(((uint64_t)m3 << 32) | m2);
    }
    for (; i < n; ++i) c += p[i] == '\n';
    return c;
}
#endif

static size_t count_newlines(const uint8_t *p, size_t n)
{
#if defined(__x86_64__)
    static const bool avx2 = __builtin_cpu_supports("avx2") && __builtin_cpu_supports("popcnt");
    if (avx2) return count_newlines_avx2(p, n);
#endif
    size_t c = 0;
    for (size_t i = 0; i < n; ++i) c += p[i] == '\n';
    return c;
}

// A compressed input as the decoders want it: all of its bytes in memory with `pad` readable zero bytes behind them.
// The file is MAPPED (its pages are touched by the decoding threads, side by side, as they reach them) in front of one
// anonymous page that provides the padding; reading 240 MB into a zero-filled vector first cost a .fq.gz of 3 M reads
// 70 ms of serial start-up before the first block was decoded.  Falls back to reading into a plain buffer.
class CompressedFile {
  public:
    CompressedFile() = default;
    CompressedFile(const CompressedFile &) = delete;
    CompressedFile &operator=(const CompressedFile &) = delete;
    ~CompressedFile()
    {
        if (map_) munmap(map_, map_len_);
        free(buf_);
    }
    bool open(const char *path, size_t pad)
    {
        const int fd = ::open(path, O_RDONLY);
        if (fd < 0) return false;
        struct stat sb;
        if (fstat(fd, &sb) != 0 || sb.st_size < 0) { ::close(fd); return false; }
        n_ = (size_t)sb.st_size;
        const size_t page = 4096, body = (n_ + page - 1) & ~(page - 1), tail = (pad + page - 1) & ~(page - 1);
        static const bool no_map = getenv("MHX_NO_MMAP") != nullptr;
        if (n_ > 0 && S_ISREG(sb.st_mode) && !no_map) {
            void *base = mmap(nullptr, body + tail, PROT_READ, MAP_PRIVATE | MAP_ANONYMOUS, -1, 0); // zero pages ...
            if (base != MAP_FAILED) {
                if (mmap(base, n_, PROT_READ, MAP_PRIVATE | MAP_FIXED, fd, 0) != MAP_FAILED) { // ... with the file laid over the front
                    map_ = base; map_len_ = body + tail; data_ = (const uint8_t *)base;
                    ::close(fd);
                    return true;
                }
                munmap(base, body + tail);
            }
        }
        buf_ = (uint8_t *)malloc(n_ + pad + 1);
        if (!buf_) { ::close(fd); return false; }
        size_t got = 0;
        while (got < n_) {
            const ssize_t r = pread(fd, buf_ + got, n_ - got, (off_t)got);
            if (r <= 0) break;
            got += (size_t)r;
        }
        ::close(fd);
        memset(buf_ + got, 0, n_ + pad - got);
        data_ = buf_;
        return got == n_;
    }
    const uint8_t *data() const { return data_; }
    size_t size() const { return n_; }

  private:
    void *map_ = nullptr;
    size_t map_len_ = 0, n_ = 0;
    uint8_t *buf_ = nullptr;
    const uint8_t *data_ = nullptr;
};

// CRC-32 of a gzip member computed BEHIND the decoder: the inflate thread hands over every piece of output as
// soon as it exists (and the trailer's expectation at a member end); this thread keeps the running CRC.
class CrcFollower {
  public:
    CrcFollower() : th_([this] { run(); }) {}
    ~CrcFollower()
    {
        { std::lock_guard<std::mutex> lk(m_); stop_ = true; }
        cv_.notify_all();
        th_.join();
    }
    void piece(const uint8_t *p, size_t n) { push({p, n, 0, false}); }
    void member_end(uint32_t expected) { push({nullptr, 0, expected, true}); }
    void drain() // everything handed over so far has been read: its buffers may go elsewhere now
    {
        std::unique_lock<std::mutex> lk(m_);
        idle_.wait(lk, [&] { return q_.empty() && !busy_; });
    }
    bool failed() { std::lock_guard<std::mutex> lk(m_); return failed_; }

  private:
    struct Item { const uint8_t *p; size_t n; uint32_t expected; bool end; };
    void push(Item it)
    {
        { std::lock_guard<std::mutex> lk(m_); q_.push_back(it); }
        cv_.notify_one();
    }
    void run()
    {
        uint32_t crc = 0;
        for (;;) {
            Item it;
            {
                std::unique_lock<std::mutex> lk(m_);
                cv_.wait(lk, [&] { return !q_.empty() || stop_; });
                if (q_.empty()) return;
                it = q_.front();
                q_.pop_front();
                busy_ = true;
            }
            bool bad = false;
            if (it.end) { bad = crc != it.expected; crc = 0; }
            else crc = crc32_update(crc, it.p, it.n);
            {
                std::lock_guard<std::mutex> lk(m_);
                busy_ = false;
                failed_ = failed_ || bad;
            }
            idle_.notify_all();
        }
    }
    std::mutex m_;
    std::condition_variable cv_, idle_;
    std::deque<Item> q_;
    bool stop_ = false, busy_ = false, failed_ = false;
    std::thread th_; // last member: started when the rest is ready
};

// Producer of one input file: inflates it (own DEFLATE decoder on the whole compressed file in memory;
// MHX_ZLIB_INFLATE=1 selects zlib's gzread instead; an uncompressed file is simply read) and cuts the
// stream into record-aligned chunks.
void inflate_fastq(const char *path, int file, bool force_zlib, int decode_threads, ChunkQueue *q, FileIngestState *st)
{
    const bool gz = is_gzip_file(path);
    const bool own = gz && !force_zlib && !getenv("MHX_ZLIB_INFLATE");
    gzFile g = nullptr;
    FILE *plain = nullptr;
    CompressedFile zfile;
    GzInflater inf;
    std::unique_ptr<CrcFollower> crc_thread; // own decoder only: the CRC pass runs beside the decoding, not after it
    // a big single-member .gz (what sequencers write) is decoded by several threads (mhx_pinflate.cpp); what follows its
    // first member, small files and anything the parallel decoder declines go through the sequential decoder
    std::unique_ptr<ParallelGunzip> par;
    size_t par_base = 0; // where in the file the member that `par` decodes begins
    std::unique_ptr<BgzfReader> bgzf; // bgzip output: independent blocks of <= 64 KiB, decoded side by side
    if (own) {
        if (!zfile.open(path, GzInflater::kInputPad)) { st->error = std::string("ERROR: could not open ") + path + " for reading"; q->producer_done(); return; }
        const size_t zn = zfile.size();
        if (decode_threads >= 2) {
            bgzf.reset(new BgzfReader());
            if (!bgzf->start(zfile.data(), zn, decode_threads)) bgzf.reset();
        }
        if (!bgzf && decode_threads >= 2) {
            par.reset(new ParallelGunzip());
            if (!par->start(zfile.data(), zn, decode_threads)) par.reset();
        }
        inf.set_input(zfile.data(), zn);
        if (!getenv("MHX_INLINE_CRC")) { inf.set_deferred_crc(true); crc_thread.reset(new CrcFollower()); }
    } else if (gz) {
        g = gzopen(path, "rb");
        if (g) gzbuffer(g, 1 << 20);
    } else {
        plain = fopen(path, "rb");
    }
    if (!own && !g && !plain) { st->error = std::string("ERROR: could not open ") + path + " for reading"; q->producer_done(); return; }
    auto close_all = [&]() { if (g) gzclose(g); if (plain) fclose(plain); };
    std::vector<uint8_t> tail; // [history in front of the carry][carry]: the end of the previous chunk's stream
    size_t carry_len = 0;
    uint64_t produced = 0;     // inflated bytes so far (bounds how far back a match may reach)
    bool first = true;
    const bool dbg = getenv("MHX_INGEST_DEBUG") != nullptr;
    double t_alloc = 0, t_inflate = 0, t_cut = 0, t_put = 0;
    auto now = []() { return std::chrono::steady_clock::now(); };
    auto secs = [](std::chrono::steady_clock::time_point a, std::chrono::steady_clock::time_point b) { return std::chrono::duration<double>(b - a).count(); };
    struct Report { bool on; const char *path; double *a, *i, *c, *p; ~Report() { if (on) fprintf(stderr, "ingest %s: alloc %.3f inflate %.3f cut %.3f put-wait %.3f s\n", path, *a, *i, *c, *p); } } report{dbg, path, &t_alloc, &t_inflate, &t_cut, &t_put};
    for (;;) {
        auto t0 = now();
        IngestChunk c;
        c.file = file;
        c.first_of_file = first;
        q->take_buffer(c);
        uint8_t *d = c.data();
        if (!tail.empty()) memcpy(d + carry_len - tail.size(), tail.data(), tail.size());
        t_alloc += secs(t0, now());
        t0 = now();
        size_t n = carry_len;
        bool eof = false;
        while (n < kIngestChunk) {
            long got;
            if (bgzf) {
                const size_t r = bgzf->read(d + n, kIngestChunk - n);
                if (r == (size_t)-1) got = -1;
                else if (r == 0) { // end of the run of BGZF blocks (each one's CRC and length verified): the rest, if any, sequentially
                    const size_t off = bgzf->consumed_input(), zn = zfile.size();
                    bgzf.reset();
                    inf.set_input(zfile.data() + off, zn - off);
                    produced = 0;
                    if (off >= zn) { eof = true; break; }
                    continue;
                } else {
                    got = (long)r;
                    produced += r;
                }
            } else if (par) {
                const size_t r = par->read(d + n, kIngestChunk - n);
                if (r == (size_t)-1) got = -1;
                else if (r == 0) { // end of a member (CRC and length verified): a further large member (`cat a.gz b.gz`) gets the
                                   // threads again, anything else goes to the sequential decoder
                    const size_t off = par_base + par->consumed_input(), zn = zfile.size();
                    par.reset();
                    produced = 0;
                    if (off < zn) {
                        par.reset(new ParallelGunzip());
                        if (par->start(zfile.data() + off, zn - off, decode_threads)) { par_base = off; continue; }
                        par.reset();
                    }
                    inf.set_input(zfile.data() + off, zn - off);
                    continue;
                } else {
                    got = (long)r;
                    produced += r;
                }
            } else if (own) {
                const uint64_t hist = produced < GzInflater::kWindow ? produced : GzInflater::kWindow;
                // pieces of 1 MiB when the CRC follows on its own thread (it reads them while they are still in cache)
                const size_t want = crc_thread ? std::min<size_t>(kIngestChunk - n, 1u << 20) : kIngestChunk - n;
                const size_t r = inf.inflate(d + n, want, d + n - hist);
                if (r == (size_t)-1) got = -1;
                else {
                    got = (long)r;
                    produced += r;
                    if (crc_thread) {
                        uint32_t expected;
                        if (r) crc_thread->piece(d + n, r);
                        if (inf.take_member_end(&expected)) crc_thread->member_end(expected);
                    }
                    if (inf.done()) { n += r; eof = true; break; }
                    if (r == 0) continue; // a member ended exactly here: the next call starts the next one
                }
            } else if (gz) {
                got = gzread(g, d + n, (unsigned)std::min<size_t>(kIngestChunk - n, 1u << 30));
            } else {
                got = (long)fread(d + n, 1, kIngestChunk - n, plain);
                if (got == 0 && ferror(plain)) got = -1;
            }
            if (got < 0) {
                if (crc_thread) crc_thread->drain(); // the follower may still be reading pieces of this chunk's buffer
                st->error = std::string("ERROR: reading ") + path + " failed";
                st->own_inflate_failed = own; // the caller repeats the run with zlib before giving up
                close_all();
                q->producer_done();
                return;
            }
            if (got == 0) { eof = true; break; }
            n += (size_t)got;
        }
        if (crc_thread) {
            crc_thread->drain(); // the follower has read everything of this chunk: it may be cut, queued and recycled
            if (crc_thread->failed()) {
                st->error = std::string("ERROR: reading ") + path + " failed";
                st->own_inflate_failed = true;
                close_all();
                q->producer_done();
                return;
            }
        }
        t_inflate += secs(t0, now());
        t0 = now();
        if (first && n && d[0] != '@') { st->not_fastq4 = true; close_all(); q->producer_done(); return; }
        // Cut in front of the last record start that can be VERIFIED inside the chunk: a line that begins with '@', is
        // followed by a line that begins with neither '@' nor '+', and then by a line that begins with '+' -- the shape
        // no quality line can imitate (a quality line may begin with '@', but the line after it is a header and begins
        // with '@' as well).  A few lines are walked back from the end of the chunk; counting all of its newlines (round
        // 2) cost this thread a third of its time.  Every chunk thus starts at a record start; the records themselves
        // are parsed, checked for the 4-line layout and counted on the device.
        size_t cut = 0;
        if (!eof) {
            size_t ls[3] = {n, n, n}; // starts of the line under test and of the two lines behind it
            const uint8_t *p = (const uint8_t *)memrchr(d, '\n', n);
            for (int walked = 0; p && walked < 4096; ++walked) {
                const uint8_t *prev = p > d ? (const uint8_t *)memrchr(d, '\n', (size_t)(p - d)) : nullptr;
                ls[2] = ls[1]; ls[1] = ls[0];
                ls[0] = (size_t)(p - d) + 1;                 // the line that starts behind newline p ...
                const size_t start = prev ? (size_t)(prev - d) + 1 : 0; // ... and the one that ends with it
                // test the line [start, p]: its two successors start at ls[0] and ls[1]
                if (ls[1] < n && d[start] == '@' && d[ls[0]] != '@' && d[ls[0]] != '+' && d[ls[1]] == '+') { cut = start; break; }
                p = prev;
            }
            if (cut == 0) st->not_fastq4 = true; // no record start in sight (a record larger than a chunk, or not 4-line FASTQ): the record parser
        } else {
            // the last chunk starts at a record start like every other: its lines must come in fours (a last record may
            // lack its final newline)
            const uint64_t lines = count_newlines(d, n) + (n && d[n - 1] != '\n' ? 1 : 0);
            if (lines & 3) st->not_fastq4 = true;
            const size_t look = std::min<size_t>(n, 1u << 16);
            if (!fastq_tail_complete(d + n - look, look)) st->not_fastq4 = true; // quality string of the last record cut short: the record parser reports it
            cut = n;
        }
        if (st->not_fastq4) { close_all(); q->producer_done(); return; }
        carry_len = n - cut;
        if (!eof) {
            // the next chunk starts with the carry; in front of it goes what is left of the 32 KiB window
            const size_t want = carry_len >= GzInflater::kWindow ? carry_len : GzInflater::kWindow;
            const size_t have = (size_t)std::min<uint64_t>(own ? produced : 0, want); // zlib keeps its own window
            const size_t keep = have > carry_len ? have : carry_len;
            tail.assign(d + n - keep, d + n);
        }
        c.size = cut;
        st->bytes += cut;
        first = false;
        t_cut += secs(t0, now());
        t0 = now();
        if (cut) q->put(std::move(c));
        t_put += secs(t0, now());
        if (eof || q->aborted()) break;
    }
    close_all();
    q->producer_done();
}

// thread entry of a producer: nothing may escape it (a failed allocation ends the file's stream with an error, not the process)
void inflate_fastq_guarded(const char *path, int file, bool force_zlib, int decode_threads, ChunkQueue *q, FileIngestState *st)
{
    try {
        inflate_fastq(path, file, force_zlib, decode_threads, q, st);
    } catch (const std::exception &e) {
        st->error = std::string("ERROR: reading ") + path + " failed (" + e.what() + ")";
        q->abort();
        q->producer_done();
    }
}

uint64_t guess_inflated_bytes(const char *path)
{
    struct stat sb;
    if (stat(path, &sb) != 0) return 0;
    return (uint64_t)sb.st_size * (is_gzip_file(path) ? 8 : 1);
}
} // namespace

// ---- bulk ingest of an uncompressed FASTQ file -------------------------------------------
// The whole file goes into ONE device buffer and ONE push: reader threads pread() disjoint
// ranges of a 64 MiB block into a pinned staging slot, the block is copied to its place in the
// device buffer on a copy stream while the next block is being read, and the device parser
// finds the records itself (line phase by look-back), so the host never scans the bytes.
namespace mhx {
// reads [off, off + len) of fd into dst with `nthreads` parallel preads; false on a short read
bool parallel_pread(int fd, uint8_t *dst, uint64_t off, size_t len, int nthreads)
{
    JoinedThreads th;
    if (nthreads < 1) nthreads = 1;
    std::vector<int> ok((size_t)nthreads, 1);
    const size_t per = ((len + (size_t)nthreads - 1) / (size_t)nthreads + 4095) & ~(size_t)4095;
    for (int t = 0; t < nthreads; ++t) {
        const size_t b = (size_t)t * per;
        if (b >= len) break;
        const size_t e = std::min(len, b + per);
        const bool last = e == len; // the calling thread reads the last part itself (all of it when there is one part)
        auto part = [=, &ok]() {
            size_t done = b;
            while (done < e) {
                const ssize_t got = pread(fd, dst + done, e - done, (off_t)(off + done));
                if (got <= 0) { ok[(size_t)t] = 0; return; }
                done += (size_t)got;
            }
        };
        if (last || !th.spawn(part)) part(); // (or no thread to be had)
    }
    th.join();
    for (int v : ok) if (!v) return false;
    return true;
}
} // namespace mhx

namespace {
constexpr size_t kBulkBlock = 64u << 20;

struct BulkFile {
    DevArray<uint8_t> d_buf;
    uint64_t size = 0;
    std::vector<uint8_t> head; // first bytes of the file (record name / comment)
    std::vector<uint8_t> tail; // its last bytes (is the last record complete?)
};

static int ensure_pinned_ring()
{
    if (!g.copy_stream) HIPCHK(hipStreamCreateWithFlags(g.copy_stream.out(), hipStreamNonBlocking));
    for (int i = 0; i < Engine::kPinnedSlots; ++i) {
        HIPCHK(g.pinned[i].grow(kBulkBlock));
        if (!g.pinned_free[i]) HIPCHK(hipEventCreateWithFlags(g.pinned_free[i].out(), hipEventDisableTiming));
    }
    return MHX_OK;
}

// MHX_OK and f->d_buf set, or MHX_OK with d_buf == nullptr when the file should take another path
static int bulk_load_plain(const char *path, BulkFile *f)
{
    struct stat sb;
    if (stat(path, &sb) != 0 || !S_ISREG(sb.st_mode) || sb.st_size <= 0) return MHX_OK;
    size_t free_b = 0, total_b = 0;
    if (hipMemGetInfo(&free_b, &total_b) != hipSuccess) return MHX_OK;
    if ((uint64_t)sb.st_size + (4ull << 30) > free_b / 2) return MHX_OK; // leave room for tables and other files
    if (ensure_pinned_ring()) { clear_error(); (void)hipGetLastError(); return MHX_OK; } // no pinned staging: the chunked path will do
    int rc = MHX_OK;
    const int fd = open(path, O_RDONLY);
    if (fd < 0) return fail(MHX_E_IO, "ERROR: could not open %s for reading", path);
    f->size = (uint64_t)sb.st_size;
    if (f->d_buf.grow(f->size + 64) != hipSuccess) { // tolerated: forget the sticky error, take the chunked path
        (void)hipGetLastError();
        close(fd);
        return MHX_OK;
    }
    int nthreads = std::min(16, ingest_thread_budget()); // pread threads: beyond 16 the page cache copy does not get faster
    uint64_t off = 0;
    int slot = 0;
    rc = MHX_OK;
    while (off < f->size && !rc) {
        const size_t len = (size_t)std::min<uint64_t>(kBulkBlock, f->size - off);
        if (hipEventSynchronize(g.pinned_free[slot]) != hipSuccess) { rc = fail(MHX_E_HIP, "pinned slot wait failed"); break; }
        uint8_t *const block = g.pinned[slot];
        if (!parallel_pread(fd, block, off, len, len >= (8u << 20) ? nthreads : 1)) { rc = fail(MHX_E_IO, "ERROR: reading %s failed", path); break; }
        if (off == 0) f->head.assign(block, block + std::min<size_t>(len, 1u << 20));
        if (off + len >= f->size) { // the last block: keep the file's last bytes (and what the block before it contributed, if this one is short)
            const size_t keep = std::min<size_t>(len, 1u << 16);
            f->tail.assign(block + len - keep, block + len);
        }
        if (hipMemcpyAsync(f->d_buf + off, block, len, hipMemcpyHostToDevice, g.copy_stream) != hipSuccess ||
            hipEventRecord(g.pinned_free[slot], g.copy_stream) != hipSuccess) { rc = fail(MHX_E_HIP, "H2D copy failed"); break; }
        off += len;
        slot = (slot + 1) % Engine::kPinnedSlots;
    }
    close(fd);
    if (!rc && hipMemsetAsync(f->d_buf + f->size, 0, 64, g.copy_stream) != hipSuccess) rc = fail(MHX_E_HIP, "memset failed");
    if (!rc && hipStreamSynchronize(g.copy_stream) != hipSuccess) rc = fail(MHX_E_HIP, "copy stream sync failed");
    if (rc) { hipStreamSynchronize(g.copy_stream); f->d_buf.reset(); }
    return rc;
}

// name / comment of the first record mash would count (sequence of at least k bytes) in `buf`; false
// when none of the records there is long enough (name / comment then hold the first header as a last resort)
static bool first_counted_header(const uint8_t *buf, size_t n, int k, std::string &name, std::string &comment)
{
    size_t p = 0;
    while (p < n) {
        const uint8_t *h_end = (const uint8_t *)memchr(buf + p, '\n', n - p);
        if (!h_end) break;
        const size_t s0 = (size_t)(h_end - buf) + 1;
        const uint8_t *s_end = s0 < n ? (const uint8_t *)memchr(buf + s0, '\n', n - s0) : nullptr;
        const size_t s1 = s_end ? (size_t)(s_end - buf) : n;
        const size_t seq_len = s1 - s0 - ((s1 > s0 && buf[s1 - 1] == '\r') ? 1 : 0); // CRLF files: the CR is not a base
        if (seq_len >= (size_t)k) { first_header(buf + p, s1 - p, name, comment); return true; }
        // skip the '+' and quality lines
        size_t q = s1 + 1;
        for (int i = 0; i < 2 && q < n; ++i) {
            const uint8_t *e = (const uint8_t *)memchr(buf + q, '\n', n - q);
            q = e ? (size_t)(e - buf) + 1 : n;
        }
        p = q;
    }
    first_header(buf, n, name, comment);
    return false;
}

// Which record names the reference: the first counted record of the lowest-numbered file that has one
// (within its first chunk); the very first header if no file has any.
struct HeaderPick {
    int file = -1;        // file that provided a counted record
    bool fallback = false;
    std::string name, comment, fb_name, fb_comment;
    void offer(int f, const uint8_t *buf, size_t n, int k)
    {
        if (file >= 0 && f > file) return;
        std::string nm, cm;
        if (first_counted_header(buf, n, k, nm, cm)) { file = f; name = nm; comment = cm; }
        else if (!fallback || f == 0) { fallback = true; fb_name = nm; fb_comment = cm; }
    }
    void result(std::string &nm, std::string &cm) const
    {
        if (file >= 0) { nm = name; cm = comment; }
        else { nm = fb_name; cm = fb_comment; }
    }
};
} // namespace

// returns MHX_OK with *handled = true when the streaming path produced the sketch;
// *handled = false means "not strict FASTQ / could not size": use the whole-file path.
static int stream_fastq_reference(const char *const *paths, int n_paths, int k, uint32_t s, uint32_t m, std::vector<uint64_t> &hashes,
                                  std::vector<uint32_t> &counts, uint64_t *kmers, uint64_t *records, std::string *fname,
                                  std::string *fcomment, bool *handled, bool force_zlib = false, mhx_screener *scr = nullptr)
{
    *handled = false;
    uint64_t expected = 0;
    for (int i = 0; i < n_paths; ++i) expected += guess_inflated_bytes(paths[i]);
    mhx_sketcher *sk = nullptr;
    int rc = mhx_sketcher_create(k, s, m, expected, &sk);
    if (rc) return rc;
    sketcher_verify_fastq(sk, true); // bulk pushes start at '@' (checked below), chunks at a record start
    rc = attach_screen(sk, scr);
    if (rc) { mhx_sketcher_destroy(sk); return rc; }
    bool fallback = false;
    HeaderPick header;
    // 1. uncompressed files: whole file -> one device buffer -> one push (see bulk_load_plain).  The buffers
    // stay on the device until the sketch is final, so that a too-small admission budget can be repaired by
    // pushing them again into a larger sketcher instead of reading the files a second time.
    std::vector<int> queued; // files that go through an inflate thread instead
    std::vector<BulkFile> resident;
    for (int i = 0; i < n_paths && !rc && !fallback; ++i) {
        if (is_gzip_file(paths[i]) || getenv("MHX_NO_BULK")) { queued.push_back(i); continue; }
        BulkFile bf;
        rc = bulk_load_plain(paths[i], &bf);
        if (rc) break;
        if (!bf.d_buf) { queued.push_back(i); continue; }
        if (bf.head.empty() || bf.head[0] != '@') fallback = true;
        if (!fastq_tail_complete(bf.tail.data(), bf.tail.size())) fallback = true; // a last record without its qualities: the record parser reports it
        if (!fallback) header.offer(i, bf.head.data(), bf.head.size(), k);
        if (!fallback) rc = mhx_sketcher_push_device(sk, bf.d_buf, bf.size, MHX_FMT_FASTQ4);
        if (hipStreamSynchronize(g.stream) != hipSuccess && !rc) rc = fail(MHX_E_HIP, "stream sync failed");
        bf.head.clear();
        resident.push_back(std::move(bf));
    }
    // 2. compressed files: one inflate thread per file (each with its share of decoding threads), 32 MiB record-aligned
    // chunks in pinned buffers; TWO device slots: chunk j is copied on the copy stream while chunk j - 1 is being parsed
    // and hashed on the engine stream.  A slot is overwritten only when the kernels of its previous chunk have completed
    // (event) AND that chunk is known to need no repair pass (sketcher_release_push) -- no whole-stream
    // synchronisation per chunk.
    std::vector<FileIngestState> st(n_paths);
    if (!rc && !fallback && !queued.empty()) {
        for (int i = 0; i < 2 && !rc; ++i) {
            if (g.ingest_slot[i].grow(kIngestChunk + GzInflater::kOvershoot + 64) != hipSuccess) rc = fail(MHX_E_HIP, "hipMalloc failed for the ingest slot");
            if (!rc && !g.ingest_copied[i] && hipEventCreateWithFlags(g.ingest_copied[i].out(), hipEventDisableTiming) != hipSuccess) rc = fail(MHX_E_HIP, "event creation failed");
            if (!rc && !g.ingest_consumed[i] && hipEventCreateWithFlags(g.ingest_consumed[i].out(), hipEventDisableTiming) != hipSuccess) rc = fail(MHX_E_HIP, "event creation failed");
        }
        if (!rc && g.ingest_word.grow(16) != hipSuccess) rc = fail(MHX_E_HIP, "hipHostMalloc failed");
        if (!rc && !g.copy_stream && hipStreamCreateWithFlags(g.copy_stream.out(), hipStreamNonBlocking) != hipSuccess) rc = fail(MHX_E_HIP, "stream creation failed");
    }
    if (!rc && !fallback && !queued.empty()) {
        ChunkQueue q(2 * queued.size() + 4);
        // (joined on every way out of this block; declared behind the queue they feed, so they are gone before it is)
        JoinedThreads threads;
        struct AbortOnExit { ChunkQueue &q; bool armed = true; ~AbortOnExit() { if (armed) { q.abort(); (void)hipStreamSynchronize(g.copy_stream); (void)hipStreamSynchronize(g.stream); } } } abort_guard{q}; // an exception in the loop below: the producers must not wait for room for ever
        for (size_t j = 0; j < queued.size(); ++j) q.producer_started();
        // decoding threads per .gz file: the host's share (ingest_thread_budget: MHX_INGEST_THREADS, else the cores this
        // process may run on divided by the ranks of the node) split over the files that are inflated side by side
        const int budget = ingest_thread_budget();
        const int per_file = std::max(1, budget / (int)std::max<size_t>(1, queued.size()) - 1);
        for (int i : queued) {
            if (threads.spawn(inflate_fastq_guarded, paths[i], i, force_zlib, per_file, &q, &st[i])) continue;
            q.producer_done(); // this file has no producer: give up on the call
            if (!rc) { rc = fail(MHX_E_INTERNAL, "could not start an ingest thread"); q.abort(); }
        }
        IngestChunk c, in_flight[2]; // in_flight[slot]: the host buffer whose copy into that slot may still be running
        uint64_t nchunk = 0;
        auto hip_ok = [&](hipError_t e, const char *what) { if (e != hipSuccess && !rc) { rc = fail(MHX_E_HIP, "%s failed: %s", what, hipGetErrorString(e)); q.abort(); } return e == hipSuccess; };
        while (q.get(c)) {
            if (rc) continue; // drain
            if (c.first_of_file) header.offer(c.file, c.data(), std::min<size_t>(c.size, 1u << 20), k);
            const int slot = (int)(nchunk & 1);
            if (nchunk >= 2) { // the slot's previous tenant (chunk nchunk - 2): kernels through, repair question settled
                if (!hip_ok(hipEventSynchronize(g.ingest_consumed[slot]), "event wait")) continue;
                rc = sketcher_release_push(sk, g.ingest_slot[slot], g.copy_stream, g.ingest_word);
                if (rc) { q.abort(); continue; }
            }
            if (!hip_ok(hipMemcpyAsync(g.ingest_slot[slot], c.data(), c.size, hipMemcpyHostToDevice, g.copy_stream), "H2D copy")) continue;
            if (!hip_ok(hipEventRecord(g.ingest_copied[slot], g.copy_stream), "event record")) continue;
            if (!hip_ok(hipStreamWaitEvent(g.stream, g.ingest_copied[slot], 0), "stream wait")) continue;
            rc = mhx_sketcher_push_device(sk, g.ingest_slot[slot], c.size, MHX_FMT_FASTQ4);
            if (rc) { q.abort(); continue; }
            if (!hip_ok(hipEventRecord(g.ingest_consumed[slot], g.stream), "event record")) continue;
            // the host buffer goes back to the producers once its copy has completed: the one of the OTHER slot has had a
            // whole chunk's time for that
            if (in_flight[slot ^ 1].buf.p) {
                if (!hip_ok(hipEventSynchronize(g.ingest_copied[slot ^ 1]), "event wait")) continue;
                in_flight[slot ^ 1].release();
            }
            in_flight[slot] = std::move(c);
            ++nchunk;
        }
        if (hipStreamSynchronize(g.copy_stream) != hipSuccess && !rc) rc = fail(MHX_E_HIP, "copy stream sync failed");
        if (rc) hipStreamSynchronize(g.stream); // nothing may still read the slots or the buffers when we leave
        in_flight[0].release();
        in_flight[1].release();
        threads.join();
        abort_guard.armed = false;
    }
    bool own_failed = false;
    for (auto &f : st) own_failed = own_failed || f.own_inflate_failed;
    if (own_failed && !force_zlib) { // the engine's own decoder refused a stream: let zlib have the last word
        resident.clear();
        mhx_sketcher_destroy(sk);
        clear_error();
        return stream_fastq_reference(paths, n_paths, k, s, m, hashes, counts, kmers, records, fname, fcomment, handled, true, scr);
    }
    for (auto &f : st) {
        if (!f.error.empty() && !rc) rc = fail(MHX_E_IO, "%s", f.error.c_str());
        if (f.not_fastq4) fallback = true;
    }
    uint32_t n = 0;
    if (!rc && !fallback) {
        hashes.resize(s);
        counts.resize(s);
        rc = mhx_sketcher_finish(sk, hashes.data(), counts.data(), &n);
        // admission budget too small (few solid k-mers: the sketch needs hashes the cap rejected): when every
        // input is still resident on the device, push it again into a sketcher with 16x, 256x ... the budget
        uint32_t scale = 1;
        while (rc == MHX_E_CAPACITY && queued.empty() && !resident.empty() && scale < (1u << 20)) {
            scale *= 16;
            clear_error();
            mhx_sketcher_destroy(sk);
            sk = nullptr;
            rc = create_sketcher(k, s, m, expected, scale, &sk);
            sketcher_verify_fastq(sk, true);
            if (!rc) rc = attach_screen(sk, scr);
            for (size_t i = 0; i < resident.size() && !rc; ++i) rc = mhx_sketcher_push_device(sk, resident[i].d_buf, resident[i].size, MHX_FMT_FASTQ4);
            if (!rc) rc = mhx_sketcher_finish(sk, hashes.data(), counts.data(), &n);
        }
        if (rc == MHX_E_FORMAT || rc == MHX_E_CAPACITY) { fallback = true; rc = MHX_OK; clear_error(); }
    }
    if (!rc && !fallback) {
        uint64_t stt[8];
        rc = mhx_sketcher_stats(sk, stt);
        *kmers = stt[0];
        header.result(*fname, *fcomment);
        if (!rc) rc = mhx_sketcher_record_count(sk, records); // sequences of >= k bytes, counted by the device parser
        hashes.resize(n);
        counts.resize(n);
        *handled = !rc;
    }
    if (sk) mhx_sketcher_destroy(sk);
    return rc;
}

// ---- FASTA through the device parser ------------------------------------------------------------------------
// `mash sketch` without -r: one reference per file (auriclass/classes.py:696-713).  The inflated file goes to the GPU
// as it is; mhx_fasta.hip squeezes it into the dense sequence stream (header lines dropped, line breaks removed inside a
// record, one separator byte in front of every record) and notes where the records start, the sketch kernel hashes the
// stream.  The host only looks at the record start positions (lengths, the count of records of >= k bases, the first
// of them for the reference's name).  Returns kFastaNotForDevice when the file is not plain FASTA (does not start
// with '>', or holds FASTQ syntax): the caller then takes the host record parser, as before.
namespace {
constexpr int kFastaNotForDevice = 1;

struct FastaInfo {
    uint64_t records = 0, total_length = 0;
    std::string first_name, first_comment;
};

// header line number `idx` (0-based, counting lines that start with '>') of a FASTA held in memory
bool nth_header(const uint8_t *b, size_t n, uint64_t idx, std::string &name, std::string &comment)
{
    size_t p = 0;
    uint64_t seen = 0;
    while (p < n) {
        const uint8_t *e = (const uint8_t *)memchr(b + p, '\n', n - p);
        const size_t le = e ? (size_t)(e - b) : n;
        if (b[p] == '>') {
            if (seen == idx) { first_header(b + p, le - p, name, comment); return true; }
            ++seen;
        }
        p = le + 1;
    }
    return false;
}
} // namespace

// device buffers of the FASTA path for files of up to n bytes (both raw buffers, the stream, the workspace), the pinned
// word block, the record positions, the two "raw bytes are in place" events
static int ensure_fasta_buffers(uint64_t n)
{
    FastaCtx &c = g.fasta;
    size_t os, oi, oo, of;
    const size_t ws_bytes = fasta_workspace_bytes(n, &os, &oi, &oo, &of);
    HIPCHK(c.h_words.grow(2 + (size_t)kFastaSepsInline));
    for (int i = 0; i < 2; ++i)
        if (!c.raw_ready[i]) HIPCHK(hipEventCreateWithFlags(c.raw_ready[i].out(), hipEventDisableTiming));
    if (c.d_raw[0].cap() < n + 64 || c.d_ws.cap() < ws_bytes) { // grow with room: the next assembly is about as large as this one
        HIPCHK(hipStreamSynchronize(g.stream));
        if (g.copy_stream) HIPCHK(hipStreamSynchronize(g.copy_stream));
        c.d_raw[0].reset(); c.d_raw[1].reset(); c.d_out.reset(); c.d_ws.reset(); // all four go before any is allocated again
        const size_t want = (size_t)(n + n / 4 + (1u << 20));
        size_t os2, oi2, oo2, of2;
        const size_t ws_want = fasta_workspace_bytes(want, &os2, &oi2, &oo2, &of2);
        // (d_ws last: after a failure it is empty, and the next call grows all four again)
        if (c.d_raw[0].grow(want + 64) || c.d_raw[1].grow(want + 64) || c.d_out.grow(want + 64) || c.d_ws.grow(ws_want))
            return fail(MHX_E_HIP, "hipMalloc failed for the FASTA buffers (%llu bytes)", (unsigned long long)n);
    }
    if (c.d_seps.grow(1u << 16) != hipSuccess) return fail(MHX_E_HIP, "hipMalloc failed for the FASTA record positions");
    return MHX_OK;
}

// One FASTA file, bytes in host memory (a pinned staging slot or a vector) -> its reference sketch.  Device buffers and the
// sketcher live in g.fasta between files and calls; two stream synchronisations per file (record layout, sketch).
// Only for files that pass fasta_for_device, with ensure_fasta_buffers(n) done.  which: the raw buffer of this file
// (d_raw[which]); on_device: the loader has already copied the bytes there on the copy stream (raw_ready[which] says when)
static bool fasta_for_device(const uint8_t *raw, uint64_t n) { return n != 0 && raw[0] == '>' && n <= 0x7FFFFFFF00ull; }
// the first half: raw bytes -> the dense stream in g.fasta.d_out (`total` bytes) and the sorted positions of the record
// separators in it (separator i sits in front of record i); *relaunches: how often the kernels ran again because the
// record list had to grow
static int fasta_stream_on_device(const uint8_t *raw, uint64_t n, int which, bool on_device, std::vector<uint64_t> &seps, uint64_t &total,
                                  uint32_t *relaunches = nullptr)
{
    FastaCtx &c = g.fasta;
    size_t os, oi, oo, of;
    fasta_workspace_bytes(n, &os, &oi, &oo, &of);
    const uint64_t ntiles = (n + kFastaTile - 1) / kFastaTile;
    uint8_t *d_raw = c.d_raw[which & 1];
    if (on_device) HIPCHK(hipStreamWaitEvent(g.stream, c.raw_ready[which & 1], 0));
    else HIPCHK(hipMemcpyAsync(d_raw, raw, n, hipMemcpyHostToDevice, g.stream));
    total = 0;
    uint32_t nsep = 0;
    for (int attempt = 0; attempt < 2; ++attempt) {
        const uint32_t seps_cap = (uint32_t)c.d_seps.cap();
        HIPCHK(launch_fasta_compact(d_raw, n, c.d_ws, c.d_out, c.d_seps, seps_cap, g.stream));
        HIPCHK(hipMemcpyAsync(&c.h_words[0], c.d_ws + oo + 8 * ntiles, 8, hipMemcpyDeviceToHost, g.stream));
        HIPCHK(hipMemcpyAsync(&c.h_words[1], c.d_ws + of, 8, hipMemcpyDeviceToHost, g.stream));
        // the record positions of an assembly (tens to hundreds of contigs) ride along with the same synchronisation
        HIPCHK(hipMemcpyAsync(&c.h_words[2], c.d_seps, (size_t)std::min(seps_cap, kFastaSepsInline) * 8, hipMemcpyDeviceToHost, g.stream));
        HIPCHK(hipStreamSynchronize(g.stream));
        total = c.h_words[0];
        uint32_t fl[2];
        memcpy(fl, &c.h_words[1], 8);
        if (fl[0] & 1u) return kFastaNotForDevice;
        nsep = fl[1];
        if (nsep <= seps_cap) break;
        if (attempt) return fail(MHX_E_INTERNAL, "FASTA record list kept growing");
        const uint32_t want = nsep + nsep / 4 + 16; // more records than there was room for: once more with room for all of them
        if (c.d_seps.grow(want) != hipSuccess) return fail(MHX_E_HIP, "hipMalloc failed for %u FASTA record positions", want);
        if (relaunches) ++*relaunches;
    }
    // records: separator i sits in front of record i; its length is the distance to the next separator (or the end)
    seps.assign(nsep, 0);
    if (nsep && nsep <= kFastaSepsInline) memcpy(seps.data(), &c.h_words[2], (size_t)nsep * 8);
    else if (nsep) {
        HIPCHK(hipMemcpyAsync(seps.data(), c.d_seps, seps.size() * 8, hipMemcpyDeviceToHost, g.stream));
        HIPCHK(hipStreamSynchronize(g.stream));
    }
    std::sort(seps.begin(), seps.end());
    return MHX_OK;
}

// Test tool: the device FASTA parser alone.  The stream comes back in out[0, *total) and the sorted separator positions in
// seps[0, *n_seps); either too small: the sizes are still reported (MHX_E_CAPACITY).  Returns kFastaNotForDevice (positive)
// for a file the file-level calls hand to the host record parser: one that does not start with '>', or FASTQ syntax.
extern "C" int mhx_fasta_stream(const void *h_bytes, uint64_t n, void *out, uint64_t cap, uint64_t *total, uint64_t *seps, uint64_t seps_cap,
                                uint64_t *n_seps, uint32_t *relaunches)
{
    return entry("mhx_fasta_stream", [&]() -> int {
        if ((!h_bytes && n) || !total || !n_seps || (!out && cap) || (!seps && seps_cap)) return fail(MHX_E_ARG, "fasta_stream: null argument");
        *total = 0; *n_seps = 0;
        if (relaunches) *relaunches = 0;
        const uint8_t *raw = (const uint8_t *)h_bytes;
        if (!fasta_for_device(raw, n)) return kFastaNotForDevice;
        int rc = ensure_fasta_buffers(n);
        if (rc) return rc;
        std::vector<uint64_t> pos;
        uint64_t tot = 0;
        rc = fasta_stream_on_device(raw, n, 0, false, pos, tot, relaunches);
        if (rc) return rc;
        *total = tot; *n_seps = pos.size();
        if (tot > cap || pos.size() > seps_cap)
            return fail(MHX_E_CAPACITY, "fasta_stream: %llu stream bytes and %zu separators need more room", (unsigned long long)tot, pos.size());
        if (tot) HIPCHK(hipMemcpy(out, g.fasta.d_out, tot, hipMemcpyDeviceToHost));
        if (!pos.empty()) memcpy(seps, pos.data(), pos.size() * 8);
        return MHX_OK;
    });
}

static int sketch_fasta_on_device(const uint8_t *raw, uint64_t n, int which, bool on_device, int k, uint32_t s, std::vector<uint64_t> &hashes, FastaInfo &info)
{
    FastaCtx &c = g.fasta;
    std::vector<uint64_t> seps;
    uint64_t total = 0;
    const int src = fasta_stream_on_device(raw, n, which, on_device, seps, total);
    if (src) return src;
    info = FastaInfo();
    uint64_t first_counted = ~0ull;
    for (size_t i = 0; i < seps.size(); ++i) {
        const uint64_t len = (i + 1 < seps.size() ? seps[i + 1] : total) - seps[i] - 1;
        if (len >= (uint64_t)k) {
            if (first_counted == ~0ull) first_counted = i;
            ++info.records;
            info.total_length += len;
        }
    }
    // a last header line without its newline has no separator and no sequence: it does not count either way
    if (info.records == 0) return MHX_OK; // the caller reports "Did not find fasta records"
    nth_header(raw, n, first_counted, info.first_name, info.first_comment);
    uint64_t boost = 1;
    for (int attempt = 0; attempt < 6; ++attempt) {
        int rc = MHX_OK;
        if (!c.sk || c.k != k || c.s != s || c.scale != boost) { // one sketcher per (k, s), reset between files
            c.sk.reset();
            mhx_sketcher *sk = nullptr;
            rc = create_sketcher(k, s, 1, 0, boost, &sk);
            if (rc) return rc;
            c.sk.reset(sk);
            c.k = k; c.s = s; c.scale = boost;
        } else {
            rc = mhx_sketcher_reset(c.sk.get());
            if (rc) return rc;
        }
        rc = mhx_sketcher_push_device(c.sk.get(), c.d_out, total, MHX_FMT_SEQ);
        uint32_t nh = 0;
        if (!rc) {
            hashes.resize(s);
            rc = mhx_sketcher_finish(c.sk.get(), hashes.data(), nullptr, &nh);
        }
        if (rc == MHX_E_CAPACITY) { boost *= 16; continue; }
        if (rc) return rc;
        hashes.resize(nh);
        return MHX_OK;
    }
    return fail(MHX_E_CAPACITY, "could not size the device table for this input");
}

// One input of `mash sketch` without -r, in host memory: an uncompressed file of up to 64 MiB is pread() straight into
// a pinned staging slot (no zero-fill, no pageable bounce on the way to the GPU), anything else is read / inflated into
// a vector.  Runs on a helper thread for file i + 1 while file i is on the GPU.
struct FastaInput {
    std::vector<uint8_t> owned;
    const uint8_t *data = nullptr;
    uint64_t n = 0;
    int slot = -1;
    bool on_device = false; // the bytes are already on their way into the file's raw buffer (raw_ready event)
    int rc = MHX_OK;
    std::string error; // (mhx_last_error is thread-local: the message travels with the input)
};

// d_dst != nullptr: the file's raw device buffer is free and large enough -- every reader thread sends what it has read
// on the copy stream right away (MiB by MiB), so the copy runs beside the reading instead of behind it
static void load_fasta_input_impl(const char *path, int slot, bool pinned_ok, FastaInput *in, uint8_t *d_dst, size_t d_cap, hipEvent_t ready);
static void load_fasta_input(const char *path, int slot, bool pinned_ok, FastaInput *in, uint8_t *d_dst, size_t d_cap, hipEvent_t ready)
{ // runs on a helper thread: nothing may escape it
    try {
        load_fasta_input_impl(path, slot, pinned_ok, in, d_dst, d_cap, ready);
    } catch (const std::exception &e) {
        in->rc = MHX_E_INTERNAL;
        in->error = std::string("reading ") + path + ": " + e.what();
    }
}

static void load_fasta_input_impl(const char *path, int slot, bool pinned_ok, FastaInput *in, uint8_t *d_dst, size_t d_cap, hipEvent_t ready)
{
    (void)hipSetDevice(g.device);
    struct stat sb;
    if (pinned_ok && !is_gzip_file(path) && stat(path, &sb) == 0 && S_ISREG(sb.st_mode) && sb.st_size > 0 && (size_t)sb.st_size + 64 <= kBulkBlock) {
        const int fd = open(path, O_RDONLY);
        if (fd >= 0) {
            bool ok = hipEventSynchronize(g.pinned_free[slot]) == hipSuccess;
            const size_t len = (size_t)sb.st_size;
            const bool stream = d_dst && len + 64 <= d_cap;
            const int nthreads = len >= (4u << 20) ? std::min(8, ingest_thread_budget()) : 1;
            uint8_t *dst = g.pinned[slot];
            JoinedThreads th;
            std::vector<int> good((size_t)nthreads, 1);
            const size_t per = ((len + (size_t)nthreads - 1) / (size_t)nthreads + 4095) & ~(size_t)4095;
            for (int t = 0; ok && t < nthreads; ++t) {
                const size_t b = (size_t)t * per;
                if (b >= len) break;
                const size_t e = std::min(len, b + per);
                auto part = [=, &good]() {
                    (void)hipSetDevice(g.device);
                    size_t done = b, sent = b;
                    while (done < e) {
                        const ssize_t got = pread(fd, dst + done, std::min<size_t>(e - done, 1u << 20), (off_t)done);
                        if (got <= 0) { good[(size_t)t] = 0; return; }
                        done += (size_t)got;
                        if (stream && (done - sent >= (1u << 20) || done == e)) {
                            if (hipMemcpyAsync(d_dst + sent, dst + sent, done - sent, hipMemcpyHostToDevice, g.copy_stream) != hipSuccess) { good[(size_t)t] = 0; return; }
                            sent = done;
                        }
                    }
                };
                if (!th.spawn(part)) part(); // no thread to be had: this one reads the part itself
            }
            th.join();
            for (int v : good) ok = ok && v;
            close(fd);
            if (ok && stream) ok = hipEventRecord(ready, g.copy_stream) == hipSuccess;
            if (ok) { in->data = dst; in->n = len; in->slot = slot; in->on_device = stream; return; }
            if (stream) (void)hipStreamSynchronize(g.copy_stream); // nothing of a failed load may still be in flight
            (void)hipGetLastError();
        }
    }
    in->rc = read_all_maybe_gz(path, in->owned);
    if (in->rc) in->error = mhx_last_error();
    in->data = in->owned.data();
    in->n = in->owned.size();
}

// The read set of a reads-mode call (all files = one mixture) through the ingest: streamed where it can be, whole files
// otherwise, the host record parser for what is not strict 4-line FASTQ.  ref receives the bottom-s sketch (hashes and
// counts), count the records of at least k bases, fname / fcomment the header of the first of them.  scr: a screener
// whose prober sees every span the sketcher sees (mhx_screen_files).
static int sketch_read_set(const char *const *paths, int n_paths, int k, uint32_t s, uint32_t m, mhx_screener *scr, RefSketch &ref,
                           uint64_t &kmers, uint64_t &count, std::string &fname, std::string &fcomment)
{
    int rc = MHX_OK;
    std::vector<Loaded> loaded(n_paths);
    g.last_fastq_route = 0;
    bool streamed = false;
    if (!getenv("MHX_NO_STREAMING")) {
        rc = stream_fastq_reference(paths, n_paths, k, s, m, ref.hashes, ref.counts, &kmers, &count, &fname, &fcomment, &streamed, false, scr);
        if (rc) return rc;
    }
    std::vector<Loaded *> in;
    if (!streamed) {
        for (int i = 0; i < n_paths; ++i) {
            rc = read_all_maybe_gz(paths[i], loaded[i].raw);
            if (rc) return rc;
            loaded[i].fastq4 = looks_like_fastq4(loaded[i].raw.data(), loaded[i].raw.size());
            in.push_back(&loaded[i]);
        }
        rc = sketch_reference(in, k, s, m, true, ref.hashes, ref.counts, &kmers, scr);
        if (rc) return rc;
    }
    // name / comment / count: the first counted record and the number of counted ones (sequence of at least
    // k bytes) -- from the record parser where it ran, from a 4-line walk over the raw bytes where the stream
    // went to the device parser untouched
    bool any = streamed;
    std::string fb_name, fb_comment;
    bool have_fb = false;
    if (streamed) g.last_fastq_route = MHX_ROUTE_DEVICE_STREAMED;
    else if (g.last_fastq_route == 0) g.last_fastq_route = MHX_ROUTE_DEVICE_WHOLE; // (sketch_reference notes the record parser)
    for (auto &l : loaded) {
        if (streamed) break;
        if (l.rec.records_seen || !l.rec.seq.empty()) {
            if (!any && l.rec.records) { fname = l.rec.first_name; fcomment = l.rec.first_comment; any = true; }
            count += l.rec.records;
        } else if (!l.raw.empty()) {
            const uint8_t *b = l.raw.data();
            const size_t n = l.raw.size();
            if (!have_fb) { first_header(b, n, fb_name, fb_comment); have_fb = true; }
            size_t p = 0;
            while (p < n) { // one record: header, sequence, '+', quality
                const uint8_t *e0 = (const uint8_t *)memchr(b + p, '\n', n - p);
                if (!e0) break;
                const size_t s0 = (size_t)(e0 - b) + 1;
                const uint8_t *e1 = s0 < n ? (const uint8_t *)memchr(b + s0, '\n', n - s0) : nullptr;
                const size_t s1 = e1 ? (size_t)(e1 - b) : n;
                const size_t len = s1 - s0 - ((s1 > s0 && b[s1 - 1] == '\r') ? 1 : 0);
                if (len >= (size_t)k) {
                    if (!any) { first_header(b + p, s1 - p, fname, fcomment); any = true; }
                    ++count;
                }
                size_t q = s1 + 1;
                for (int i = 0; i < 2 && q < n; ++i) {
                    const uint8_t *e = (const uint8_t *)memchr(b + q, '\n', n - q);
                    q = e ? (size_t)(e - b) + 1 : n;
                }
                p = q;
            }
        }
    }
    if (!any && have_fb) { fname = fb_name; fcomment = fb_comment; }
    return MHX_OK;
}

// `mash sketch -i`: one reference per RECORD.  Either route lays a file out as a dense stream plus record offsets and ends
// in the segmented sketch (mhx_engine_segments.cpp): plain FASTA through the device parser, whose separator positions are
// the offsets (the separator byte in front of a record is a newline: part of the segment, never of a window); anything
// else through the host record parser.  Records shorter than k are left out; a file from which none remains fails as it
// does in the per-file mode.
namespace {
// every header line of a plain FASTA held in memory, in order (header i belongs to separator i of the device parser)
void fasta_headers(const uint8_t *b, size_t n, std::vector<std::string> &names, std::vector<std::string> &comments)
{
    size_t p = 0;
    while (p < n) {
        const uint8_t *e = (const uint8_t *)memchr(b + p, '\n', n - p);
        const size_t le = e ? (size_t)(e - b) : n;
        if (b[p] == '>') {
            names.emplace_back();
            comments.emplace_back();
            first_header(b + p, le - p, names.back(), comments.back());
        }
        p = le + 1;
    }
}

constexpr uint64_t kIndividualRowsRound = 64ull << 20; // bytes of result rows on the host at a time

// The records of one file -- record i = [off[i] + lead, off[i + 1]) of the stream, which lies on the device (d_stream) or on
// the host (h_stream) -- sketched in rounds and appended to `set`; returns the number of references added in *added.
int sketch_records(const uint8_t *d_stream, const uint8_t *h_stream, uint64_t stream_n, const std::vector<uint64_t> &off, uint64_t lead,
                   const std::vector<std::string> &names, const std::vector<std::string> &comments, int k, uint32_t s, SketchSet &set,
                   uint64_t *added)
{
    *added = 0;
    const size_t nrec = off.empty() ? 0 : off.size() - 1;
    if (nrec > 0x7FFFFFFFull) return fail(MHX_E_ARG, "too many records in one file (%zu)", nrec);
    uint64_t max_w = 0;
    for (size_t i = 0; i < nrec; ++i) max_w = std::max<uint64_t>(max_w, off[i + 1] - off[i] >= (uint64_t)k ? off[i + 1] - off[i] - (uint64_t)k + 1 : 0);
    const uint32_t stride = (uint32_t)std::min<uint64_t>(s, max_w);
    if (stride == 0) return MHX_OK; // no record of k bytes
    const size_t per_round = (size_t)std::max<uint64_t>(1, kIndividualRowsRound / ((uint64_t)stride * sizeof(uint64_t)));
    std::vector<uint64_t> rows;
    std::vector<uint32_t> len;
    for (size_t i0 = 0; i0 < nrec; i0 += per_round) {
        const uint32_t cnt = (uint32_t)std::min(per_round, nrec - i0);
        rows.resize((size_t)cnt * stride);
        len.resize(cnt);
        const int rc = d_stream ? segments_resident(d_stream, off.data() + i0, cnt, k, s, stride, rows.data(), len.data())
                                : mhx_sketch_segments(h_stream, stream_n, off.data() + i0, cnt, k, s, rows.data(), len.data(), stride, 0);
        if (rc) return rc;
        for (uint32_t j = 0; j < cnt; ++j) {
            const size_t i = i0 + j;
            const uint64_t length = off[i + 1] - off[i] - lead;
            if (off[i + 1] - off[i] < lead || length < (uint64_t)k) continue; // mash does not count a record shorter than k
            RefSketch ref;
            if (i < names.size()) { ref.name = names[i]; ref.comment = comments[i]; }
            ref.length = length;
            ref.hashes.assign(rows.data() + (size_t)j * stride, rows.data() + (size_t)j * stride + len[j]);
            set.refs.push_back(std::move(ref));
            ++*added;
        }
    }
    return MHX_OK;
}
} // namespace

extern "C" int mhx_sketch_files_individual(const char *const *paths, int n_paths, int k, uint32_t s, const char *out_msh, char *stderr_buf,
                                           size_t stderr_cap, size_t *stderr_need, uint64_t *n_refs_out)
{
    return entry("mhx_sketch_files_individual", [&]() -> int {
        int rc = MHX_OK;
        if (!paths || n_paths <= 0 || !out_msh) return fail(MHX_E_ARG, "sketch: paths and output required");
        for (int i = 0; i < n_paths; ++i)
            if (!paths[i]) return fail(MHX_E_ARG, "sketch: input path %d is null", i);
        if (!hash_k_supported(k)) return fail(MHX_E_ARG, "k-mer size %d not supported (1..32)", k);
        if (s == 0) return fail(MHX_E_ARG, "sketch: sketch size 0");
        SketchSet set;
        set.kmer_size = (uint32_t)k;
        set.sketch_size = s;
        std::string err;
        std::vector<uint8_t> raw;
        for (int i = 0; i < n_paths; ++i) {
            err += std::string("Sketching ") + paths[i] + "...\n";
            rc = read_all_maybe_gz(paths[i], raw);
            if (rc) return rc;
            uint64_t added = 0;
            bool done = false;
            if (!getenv("MHX_HOST_FASTA") && fasta_for_device(raw.data(), raw.size())) { // plain FASTA: parsed on the device
                rc = ensure_fasta_buffers(raw.size());
                if (rc) return rc;
                std::vector<uint64_t> off;
                uint64_t total = 0;
                rc = fasta_stream_on_device(raw.data(), raw.size(), 0, false, off, total);
                if (rc < 0) return rc;
                if (rc == MHX_OK) {
                    off.push_back(total);
                    std::vector<std::string> names, comments;
                    fasta_headers(raw.data(), raw.size(), names, comments);
                    rc = sketch_records(g.fasta.d_out, nullptr, total, off, 1, names, comments, k, s, set, &added);
                    if (rc) return rc;
                    done = true;
                }
            }
            if (!done) { // FASTQ, a file that does not start with '>', ...: the host record parser
                RecordList rec;
                rc = parse_fastx_records(raw.data(), raw.size(), rec);
                if (rc) return rc;
                if (rec.off.empty()) rec.off.push_back(0);
                rc = sketch_records(nullptr, rec.seq.data(), rec.seq.size(), rec.off, 0, rec.name, rec.comment, k, s, set, &added);
                if (rc) return rc;
            }
            if (added == 0) {
                err += std::string("ERROR: Did not find fasta records in \"") + paths[i] + "\".\n";
                put_text(err, stderr_buf, stderr_cap, stderr_need);
                return fail(MHX_E_NO_RECORDS, "ERROR: Did not find fasta records in \"%s\".", paths[i]);
            }
        }
        err += std::string("Writing to ") + out_msh + "...\n";
        rc = msh_write_file(out_msh, set);
        if (rc) return rc;
        if (n_refs_out) *n_refs_out = set.refs.size();
        return put_text(err, stderr_buf, stderr_cap, stderr_need);
    });
}

// `mash screen REF.msh reads...`: the reference sketches become a screen table on the device (mhx_screen.h), the read set
// goes through the ingest of a reads-mode sketch -- with the reference file's k and sketch size and m = 1, which is the
// bottom-s sketch mash keeps beside the counting for the set size -- and the screener's prober sees every span on its
// way (sketch_read_set).  Tally on the device (opts->winner: winner-take-all), columns and the -i / -v filters on the host.
struct ScreenerDestroy { void operator()(mhx_screener *sc) const { mhx_screener_destroy(sc); } };

extern "C" int mhx_screen_files_opts(const char *ref_msh, const char *const *paths, int n_paths, const mhx_screen_opts *opts, char *stdout_buf,
                                     size_t cap, size_t *need, double *set_size_out)
{
    return entry("mhx_screen_files", [&]() -> int {
        bool winner = false;
        double min_identity = -1.0, max_p = 1.0;
        if (opts) {
            if (opts->struct_size != sizeof(mhx_screen_opts)) return fail(MHX_E_ARG, "screen: mhx_screen_opts of %u bytes, expected %zu", opts->struct_size, sizeof(mhx_screen_opts));
            if (!(opts->min_identity <= 1.0)) return fail(MHX_E_ARG, "screen: minimum identity must be at most 1");
            if (!(opts->max_p_value >= 0.0 && opts->max_p_value <= 1.0)) return fail(MHX_E_ARG, "screen: maximum p-value must be within [0, 1]");
            winner = opts->winner != 0; min_identity = opts->min_identity; max_p = opts->max_p_value;
        }
        if (!ref_msh || !paths || n_paths <= 0) return fail(MHX_E_ARG, "screen: a reference sketch path and at least one read file required");
        for (int i = 0; i < n_paths; ++i)
            if (!paths[i]) return fail(MHX_E_ARG, "screen: read file path %d is null", i);
        SketchSet R;
        int rc = msh_read_file(ref_msh, R);
        if (rc) return rc;
        if (R.hash_seed != 42) return fail(MHX_E_MISMATCH, "ERROR: The reference sketches use hash seed %u; reads are hashed with seed 42", R.hash_seed);
        if (R.alphabet != "ACGT" || R.noncanonical) return fail(MHX_E_MISMATCH, "ERROR: The reference sketches are not canonical nucleotide sketches");
        const int k = (int)R.kmer_size;
        if (!hash_k_supported(k)) return fail(MHX_E_ARG, "k-mer size %d not supported (1..32)", k);
        const uint32_t nr = (uint32_t)R.refs.size();
        uint32_t stride = 1, s_ref = R.sketch_size;
        std::vector<uint32_t> len(nr);
        for (uint32_t i = 0; i < nr; ++i) {
            if (!check_ascending(R.refs[i].hash_data(), R.refs[i].hash_count()))
                return fail(MHX_E_FORMAT, "%s: hash list of reference %u is not ascending", ref_msh, i);
            len[i] = (uint32_t)R.refs[i].hash_count();
            stride = std::max(stride, len[i]);
        }
        s_ref = std::max<uint32_t>(std::max(s_ref, stride), 1);
        std::vector<uint64_t> rows((size_t)nr * stride, 0);
        for (uint32_t i = 0; i < nr; ++i)
            if (len[i]) memcpy(rows.data() + (size_t)i * stride, R.refs[i].hash_data(), (size_t)len[i] * sizeof(uint64_t));
        mhx_screener *raw = nullptr;
        rc = mhx_screener_create(k, rows.data(), len.data(), nr, stride, s_ref, 0, 0, &raw);
        if (rc) return rc;
        std::unique_ptr<mhx_screener, ScreenerDestroy> scr(raw);
        RefSketch mix;
        uint64_t kmers = 0, count = 0;
        std::string fname, fcomment;
        rc = sketch_read_set(paths, n_paths, k, s_ref, 1, scr.get(), mix, kmers, count, fname, fcomment);
        if (rc) return rc;
        // (no record of k bases at all: mash warns and prints its rows; the sketch is empty and the set size 0)
        const double set_size = set_size_estimate(k, mix.hashes.data(), mix.hashes.size());
        std::vector<uint32_t> shared(nr), median(nr);
        if (winner) {
            std::vector<uint64_t> length(nr);
            for (uint32_t i = 0; i < nr; ++i) length[i] = R.refs[i].length;
            rc = mhx_screener_finish_winner(scr.get(), length.data(), shared.data(), median.data(), nullptr, nullptr);
        } else {
            rc = mhx_screener_finish(scr.get(), shared.data(), median.data(), nullptr, nullptr);
        }
        if (rc) return rc;
        std::string text;
        for (uint32_t i = 0; i < nr; ++i) {
            const double identity = mhx_screen_identity(shared[i], len[i], k), p = mhx_screen_p_value(shared[i], len[i], set_size, k);
            // mash screen -i / -v: -i 0 keeps identities above zero only, -i -1 everything
            if (!(min_identity == 0.0 ? identity > 0.0 : identity >= min_identity) || !(p <= max_p)) continue;
            text += fmt_g(identity) + "\t" + std::to_string(shared[i]) + "/" + std::to_string(len[i]) + "\t" + std::to_string(median[i]) + "\t" +
                    fmt_g(p) + "\t" + R.refs[i].name + "\t" + R.refs[i].comment + "\n";
        }
        if (set_size_out) *set_size_out = set_size;
        return put_text(text, stdout_buf, cap, need);
    });
}

extern "C" int mhx_screen_files(const char *ref_msh, const char *const *paths, int n_paths, char *stdout_buf, size_t cap, size_t *need,
                                double *set_size_out)
{
    return mhx_screen_files_opts(ref_msh, paths, n_paths, nullptr, stdout_buf, cap, need, set_size_out);
}

extern "C" int mhx_msh_write(const char *path, int k, uint32_t s, uint32_t n_refs, const char *const *names,
                             const char *const *comments, const uint64_t *lengths, const uint64_t *const *hashes,
                             const uint32_t *n_hashes)
{
    clear_error();
    if (!path || (n_refs && (!names || !comments || !lengths || !hashes || !n_hashes))) return fail(MHX_E_ARG, "null argument");
    return guarded("mhx_msh_write", [&] {
        SketchSet set;
        set.kmer_size = (uint32_t)k;
        set.sketch_size = s;
        set.refs.resize(n_refs);
        for (uint32_t i = 0; i < n_refs; ++i) {
            set.refs[i].name = names[i] ? names[i] : "";
            set.refs[i].comment = comments[i] ? comments[i] : "";
            set.refs[i].length = lengths[i];
            if (n_hashes[i]) set.refs[i].hashes.assign(hashes[i], hashes[i] + n_hashes[i]);
        }
        return msh_write_file(path, set);
    });
}

extern "C" int mhx_sketch_files(const char *const *paths, int n_paths, int k, uint32_t s, int reads, uint32_t min_mult,
                                const char *out_msh, char *stderr_buf, size_t stderr_cap, size_t *stderr_need,
                                double *est_genome_size)
{
    return entry("mhx_sketch_files", [&]() -> int {
        int rc = MHX_OK;
        if (!paths || n_paths <= 0 || !out_msh) return fail(MHX_E_ARG, "sketch: paths and output required");
        if (!hash_k_supported(k)) return fail(MHX_E_ARG, "k-mer size %d not supported (1..32)", k);
        SketchSet set;
        set.kmer_size = (uint32_t)k;
        set.sketch_size = s;
        std::string err;
        std::vector<Loaded> loaded(n_paths);
        auto no_records = [&](const char *p) {
            err += std::string("ERROR: Did not find fasta records in \"") + p + "\".\n";
            put_text(err, stderr_buf, stderr_cap, stderr_need);
            return fail(MHX_E_NO_RECORDS, "ERROR: Did not find fasta records in \"%s\".", p);
        };
        if (reads) {
            RefSketch ref;
            uint64_t kmers = 0, count = 0;
            std::string fname, fcomment;
            rc = sketch_read_set(paths, n_paths, k, s, min_mult ? min_mult : 1, nullptr, ref, kmers, count, fname, fcomment);
            if (rc) return rc;
            // mash stops when no record holds k bases.  (`kmers` is not that question: the device counts every window of k BYTES
            // inside one line, and a CRLF file of reads one base shorter than k has such windows -- 31 bases and the '\r' --
            // although none of them is a k-mer.)
            if (count == 0) return no_records(paths[0]);
            double set_size = 0.0, mult = 0.0;
            if (!ref.hashes.empty()) {
                set_size = pow(2.0, k > 16 ? 64.0 : 32.0) * (double)ref.hashes.size() / (double)ref.hashes.back();
                uint64_t sum = 0;
                for (uint32_t c : ref.counts) sum += c;
                mult = (double)sum / (double)ref.hashes.size();
            }
            ref.name = paths[0];
            ref.comment = make_comment(fname, fcomment, count);
            ref.length = (uint64_t)set_size;
            ref.counts.clear(); // mash stores counts only with -M
            set.refs.push_back(std::move(ref));
            err += "Estimated genome size: " + fmt_g(set_size) + "\n";
            err += "Estimated coverage:    " + fmt_g(mult) + "\n";
            if (est_genome_size) *est_genome_size = set_size;
        } else {
            // one reference per file; file i + 1 is read (and inflated) on a helper thread while file i is on the GPU
            const bool pinned_ok = !getenv("MHX_HOST_FASTA") && ensure_pinned_ring() == MHX_OK;
            if (!pinned_ok) { clear_error(); (void)hipGetLastError(); }
            std::vector<FastaInput> inputs(n_paths);
            // the device buffers are sized for the largest uncompressed input up front, so that a loader can copy file i + 1
            // into its raw buffer while file i is still on the GPU
            uint64_t largest = 0;
            for (int i = 0; i < n_paths; ++i) {
                struct stat sb;
                if (stat(paths[i], &sb) == 0 && S_ISREG(sb.st_mode) && !is_gzip_file(paths[i])) largest = std::max<uint64_t>(largest, (uint64_t)sb.st_size);
            }
            bool stream_ok = pinned_ok && largest > 0 && largest + 64 <= kBulkBlock && ensure_fasta_buffers(largest) == MHX_OK;
            if (!stream_ok) clear_error();
            auto raw_of = [&](int i) { return stream_ok ? g.fasta.d_raw[i & 1] : (uint8_t *)nullptr; };
            std::thread loader;
            struct Joiner { std::thread &t; ~Joiner() { if (t.joinable()) t.join(); } } joiner{loader};
            auto start_loader = [&](int j) { // file j on its way while file j - 1 is on the GPU; without a thread to be had: loaded here and now
                try {
                    loader = std::thread(load_fasta_input, paths[j], j % Engine::kPinnedSlots, pinned_ok, &inputs[j], raw_of(j), g.fasta.d_raw[j & 1].cap(), (hipEvent_t)g.fasta.raw_ready[j & 1]);
                } catch (const std::system_error &) {
                    load_fasta_input(paths[j], j % Engine::kPinnedSlots, pinned_ok, &inputs[j], raw_of(j), g.fasta.d_raw[j & 1].cap(), g.fasta.raw_ready[j & 1]);
                }
            };
            load_fasta_input(paths[0], 0, pinned_ok, &inputs[0], raw_of(0), g.fasta.d_raw[0].cap(), g.fasta.raw_ready[0]);
            for (int i = 0; i < n_paths; ++i) {
                if (loader.joinable()) loader.join();
                FastaInput &in = inputs[i];
                err += std::string("Sketching ") + paths[i] + "...\n";
                if (in.rc) return fail(in.rc, "%s", in.error.c_str());
                // The FASTA device buffers regrow only while no loader holds one of them: file i's are sized here, before file
                // i + 1's loader is handed its raw buffer.  Bytes that went to a buffer that has since been regrown are copied
                // again from the host.
                const bool device_parser = !getenv("MHX_HOST_FASTA") && fasta_for_device(in.data, in.n);
                if (device_parser) {
                    const size_t raw_cap = g.fasta.d_raw[i & 1].cap();
                    rc = ensure_fasta_buffers(in.n);
                    if (rc) return rc;
                    if (g.fasta.d_raw[i & 1].cap() != raw_cap) in.on_device = false;
                }
                if (i + 1 < n_paths) start_loader(i + 1);
                if (device_parser) { // plain FASTA: parsed on the device
                    RefSketch ref;
                    FastaInfo info;
                    rc = sketch_fasta_on_device(in.data, in.n, i, in.on_device, k, s, ref.hashes, info);
                    if (rc < 0) return rc;
                    if (rc == MHX_OK) {
                        if (info.records == 0) return no_records(paths[i]);
                        ref.name = paths[i];
                        ref.comment = make_comment(info.first_name, info.first_comment, info.records);
                        ref.length = info.total_length;
                        set.refs.push_back(std::move(ref));
                        in = FastaInput();
                        continue;
                    }
                }
                if (in.slot >= 0) in.owned.assign(in.data, in.data + in.n); // the record parser path keeps the bytes beyond this slot's turn
                loaded[i].raw.swap(in.owned);
                in = FastaInput();
                rc = parse_fastx(loaded[i].raw.data(), loaded[i].raw.size(), k, loaded[i].rec);
                if (rc) return rc;
                if (loaded[i].rec.records == 0) return no_records(paths[i]);
                RefSketch ref;
                std::vector<Loaded *> in2{&loaded[i]};
                rc = sketch_reference(in2, k, s, 1, false, ref.hashes, ref.counts, nullptr);
                if (rc) return rc;
                ref.counts.clear();
                ref.name = paths[i];
                ref.comment = make_comment(loaded[i].rec.first_name, loaded[i].rec.first_comment, loaded[i].rec.records);
                ref.length = loaded[i].rec.total_length;
                set.refs.push_back(std::move(ref));
                loaded[i] = Loaded();
            }
            if (est_genome_size) *est_genome_size = 0.0;
        }
        err += std::string("Writing to ") + out_msh + "...\n";
        rc = msh_write_file(out_msh, set);
        if (rc) return rc;
        return put_text(err, stderr_buf, stderr_cap, stderr_need);
    });
}

extern "C" int mhx_last_fastq_route(void) { return g.last_fastq_route; }
