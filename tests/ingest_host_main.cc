// The host side of the ingest (csrc/pdt_ingest.h) on a machine without a GPU: the layout table, the cpulist parser, the read
// loop and the page-cache probe, and the ring of slots run over a copier that is a late, out-of-order memcpy.
// tests/test_ingest_host.py builds this once with the address and undefined-behaviour sanitizers and once with the thread
// sanitizer and runs both.  argv[1]: a directory for temporary files.
#include "../project-desert-tortoise_amd/csrc/pdt_ingest.h"

#include <fcntl.h>
#include <signal.h>

#include <string>

using namespace pdtrt;

#define CHECK(cond)                                                              \
    do {                                                                         \
        if (!(cond)) {                                                           \
            fprintf(stderr, "%s:%d: CHECK failed: %s\n", __FILE__, __LINE__, #cond); \
            exit(1);                                                             \
        }                                                                        \
    } while (0)

static std::string g_dir;
static const size_t MiB = (size_t)1 << 20;

static unsigned char pattern(size_t i) { return (unsigned char)((i * 2654435761u) >> 13); }

// a file of `junk` bytes followed by pattern(0 .. n)
static int pattern_file(size_t junk, size_t n, int flags = O_RDONLY)
{
    std::string path = g_dir + "/ingest_XXXXXX";
    const int w = mkstemp(&path[0]);
    CHECK(w >= 0);
    std::vector<unsigned char> b(junk + n, 0xEE);
    for (size_t i = 0; i < n; i++) b[junk + i] = pattern(i);
    CHECK(write(w, b.data(), b.size()) == (ssize_t)b.size());
    close(w);
    const int fd = open(path.c_str(), flags);
    CHECK(fd >= 0);
    unlink(path.c_str());
    return fd;
}

// ------------------------------------------------------------------ a. the layout, by hand from the expressions of ingest_layout
static void test_layout()
{
    // 3.6e9 bytes from a file, 256 hardware threads, one context: 8 MiB spans from 512 MiB on, ceil(3.6e9 / 8388608) = 430;
    // share = max(2, 128 / 1), t_max = min(8, 128) = 8, readers = min(min(129, 8), 430) = 8
    IngestLayout L = ingest_layout(3600000000u, false, false, 0, 0, 0, 256, 1);
    CHECK(L.span == 8 * MiB && L.nspans == 430 && L.readers == 8 && L.nslots == 16 && L.streams == 4 && !L.plain_copy);
    CHECK(L.slot_stride(false) == 8 * MiB && L.slot_stride(true) == 8 * MiB + 8192);
    // 12 MiB, 32 hardware threads, 8 contexts: share = max(2, 16 / 8) = 2 = t_max, readers = min(min(17, 2), 6) = 2
    L = ingest_layout(12 * MiB, false, false, 0, 0, 0, 32, 8);
    CHECK(L.span == 2 * MiB && L.nspans == 6 && L.readers == 2 && L.nslots == 4 && L.streams == 1 && !L.plain_copy);
    // hardware_concurrency unknown: share = max(2, 8), t_max = 8, readers = min(min(4, 8), 50) = 4
    CHECK(ingest_layout(100 * MiB, false, false, 0, 0, 0, 0, 1).readers == 4);
    // 2 hardware threads: share = max(2, 1) = 2 = t_max, readers = min(min(2, 2), 50) = 2
    CHECK(ingest_layout(100 * MiB, false, false, 0, 0, 0, 2, 1).readers == 2);
    // ingest_threads = 128 on 16 hardware threads: readers = min(min(9, 128), 128) = 9
    L = ingest_layout(1024 * MiB, false, false, 128, 0, 0, 16, 1);
    CHECK(L.nspans == 128 && L.readers == 9 && L.nslots == 18 && L.streams == 4);
    // from memory: at most two spans and no job take the plain copy
    CHECK(ingest_layout(4 * MiB, true, false, 0, 0, 0, 16, 1).plain_copy);
    L = ingest_layout(4 * MiB, true, false, 0, 1, 0, 16, 1);
    CHECK(L.nspans == 4 && !L.plain_copy);
    CHECK(!ingest_layout(4 * MiB, true, true, 0, 0, 0, 16, 1).plain_copy);
    CHECK(!ingest_layout(4 * MiB, false, false, 0, 0, 0, 16, 1).plain_copy);
    // the streams tuning is clamped to 1 .. 4; one span has one reader
    CHECK(ingest_layout(100 * MiB, false, false, 0, 0, 9, 16, 1).streams == 4 && ingest_layout(1024 * MiB, false, false, 0, 0, 2, 16, 1).streams == 2);
    CHECK(ingest_layout(1000, false, false, 0, 0, 0, 16, 1).readers == 1);
    // marks: the spans of a prefix, never more than there are
    L = ingest_layout(12 * MiB + 5, false, false, 0, 0, 0, 32, 1);
    CHECK(L.nspans == 7);
    CHECK(L.mark_spans(1) == 1 && L.mark_spans(2 * MiB) == 1 && L.mark_spans(2 * MiB + 1) == 2);
    CHECK(L.mark_spans(12 * MiB + 5) == 7 && L.mark_spans(100 * MiB) == 7);
    CHECK(ingest_error(0) == PDT_OK && ingest_error(INGEST_DEVICE) == PDT_ERR_NOGPU && ingest_error(INGEST_SHORT) == PDT_ERR_FORMAT &&
          ingest_error(INGEST_READ) == PDT_ERR_IO);
}

// ------------------------------------------------------------------ b. cpulist
static void test_cpulist()
{
    cpu_set_t s;
    CHECK(parse_cpulist("0-3,8,10-11\n", &s) && CPU_COUNT(&s) == 7);
    for (int c : { 0, 1, 2, 3, 8, 10, 11 }) CHECK(CPU_ISSET(c, &s));
    CHECK(parse_cpulist("5\n", &s) && CPU_COUNT(&s) == 1 && CPU_ISSET(5, &s));
    CHECK(!parse_cpulist("", &s) && CPU_COUNT(&s) == 0);
    CHECK(!parse_cpulist("0-", &s) && CPU_COUNT(&s) == 0);
    char past[64];
    snprintf(past, sizeof past, "%d-%d\n", CPU_SETSIZE - 4, CPU_SETSIZE + 1000);
    CHECK(parse_cpulist(past, &s) && CPU_COUNT(&s) == 4 && CPU_ISSET(CPU_SETSIZE - 1, &s));
    snprintf(past, sizeof past, "%d\n", CPU_SETSIZE);
    CHECK(!parse_cpulist(past, &s));
}

// ------------------------------------------------------------------ c. the read loop and the probe
static void test_read_and_probe()
{
    const size_t page = (size_t)sysconf(_SC_PAGESIZE), n = 300 * page;
    const int fd = pattern_file(0, n);
    std::vector<unsigned char> buf(3 * page, 0xAA);
    CHECK(read_fully(fd, buf.data(), 1000, 1000, 123) == 0);
    for (size_t i = 0; i < 1000; i++) CHECK(buf[i] == pattern(123 + i));
    CHECK(buf[1000] == 0xAA);                                        // the exact fill
    CHECK(read_fully(fd, buf.data(), 2 * page, page + 5, n - 2 * page) == 0);      // (may take more than it needs, never more than `want`)
    for (size_t i = 0; i < page + 5; i++) CHECK(buf[i] == pattern(n - 2 * page + i));
    CHECK(buf[2 * page] == 0xAA);
    CHECK(read_fully(fd, buf.data(), 2 * page, page + 1, n - page) == INGEST_SHORT);
    CHECK(read_fully(fd, buf.data(), 10, 10, n) == INGEST_SHORT);
    CHECK(read_fully(-1, buf.data(), 10, 10, 0) == INGEST_READ);
    CHECK(read_fully(fd, buf.data(), 0, 0, 0) == 0);
    const double r = file_resident_fraction(fd, 4099, n - 4099);
    CHECK(r >= 0.0 && r <= 1.0);
    CHECK(file_resident_fraction(fd, 0, 63 * page) == 1.0);           // too small to be worth a probe
    CHECK(file_resident_fraction(-1, 0, n) == 1.0);
    close(fd);
    // mid-interval samples: with npages a multiple of 64, sample k is page (2k + 1) * npages / 128
    for (size_t m : { (size_t)1, (size_t)3, (size_t)4, (size_t)100, (size_t)13733 })
        for (int k = 0; k < PDT_PROBE_SAMPLES; k++) CHECK(probe_sample_page(k, 64 * m) == (size_t)(2 * k + 1) * 64 * m / 128);
    for (size_t npages : { (size_t)64, (size_t)65, (size_t)127, (size_t)1000, (size_t)878907 })
        for (int k = 0; k < PDT_PROBE_SAMPLES; k++) {
            CHECK(probe_sample_page(k, npages) < npages);
            CHECK(k == 0 || probe_sample_page(k, npages) > probe_sample_page(k - 1, npages));
        }
    CHECK(probe_sample_page(0, 1000) == 7);                          // (not page 0)
}

// ------------------------------------------------------------------ d, e. the ring
// A copy "completes" -- the bytes move -- when its slot has been polled a few times (a number that changes from copy to copy), or
// when the ring blocks on it: late, and across the streams out of order.
struct MemCopier {
    IngestJob *J;
    unsigned char *dst;
    int fail_at;                                 // the n-th copy is refused (-1: none)
    struct Flying { const unsigned char *from = nullptr; size_t at = 0, len = 0; int polls = 0; bool on = false; };
    std::vector<Flying> slot;
    std::vector<size_t> order;                   // the spans as they were queued
    std::vector<char> was_queued, mark_ok;       // per span; per mark: all spans of its prefix had been queued when it was recorded
    std::vector<int> last_stream;
    unsigned tick = 0;
    bool device_set = false;

    MemCopier(IngestJob *job, unsigned char *d, int fail) : J(job), dst(d), fail_at(fail), slot((size_t)job->lay.nslots), was_queued(job->lay.nspans, 0),
                                                           mark_ok(job->mark_spans.size(), 0) {}
    bool set_device() { device_set = true; return true; }
    bool queue(int s, int q, size_t at, const unsigned char *from, size_t len)
    {
        CHECK(device_set && q >= 0 && q < J->lay.streams && !slot[(size_t)s].on);
        CHECK(last_stream.empty() || q == (last_stream.back() + 1) % J->lay.streams);        // round robin
        if ((int)order.size() == fail_at) return false;
        const size_t k = at / J->lay.span;
        CHECK(at % J->lay.span == 0 && k < J->lay.nspans && !was_queued[k] && len == std::min(J->lay.span, J->bytes - at));
        slot[(size_t)s] = Flying{ from, at, len, (int)((tick++ * 7u + (unsigned)s) % 5u), true };
        order.push_back(k);
        was_queued[k] = 1;
        last_stream.push_back(q);
        return true;
    }
    int done(int s, bool block)
    {
        Flying &f = slot[(size_t)s];
        CHECK(f.on);
        if (!block && f.polls-- > 0) return 0;
        memcpy(dst + f.at, f.from, f.len);
        f.on = false;
        return 1;
    }
    bool mark(size_t m)
    {
        char ok = 1;
        for (size_t k = 0; k < J->mark_spans[m]; k++) ok &= was_queued[k];
        CHECK(m == 0 || mark_ok[m - 1]);                             // in order
        mark_ok[m] = ok;
        return true;
    }
    void finish()                                                    // what a stream that waits for the copies would see
    {
        for (Flying &f : slot)
            if (f.on) { memcpy(dst + f.at, f.from, f.len); f.on = false; }
    }
};

enum { SRC_MEM, SRC_FILE, SRC_FILE_DIRECT };
struct RingCase {
    size_t bytes, span;
    int readers, streams;
    bool background;
    int source;
    uint64_t off = 0;            // of the capture's first byte in the file
    size_t missing = 0;          // bytes the file is shorter than announced
    bool write_only = false;     // a descriptor whose reads fail
    int fail_at = -1;
    int expect = PDT_OK;
};

static void run_ring(const RingCase &c)
{
    alarm(20);                                                       // a lost wake-up ends the program, it does not hang it
    std::vector<unsigned char> want(c.bytes), got(c.bytes, 0x55);
    for (size_t i = 0; i < c.bytes; i++) want[i] = pattern(i);
    IngestLayout L;
    L.span = c.span;
    L.nspans = (c.bytes + c.span - 1) / c.span;
    L.readers = (int)std::min<size_t>((size_t)c.readers, L.nspans);
    L.nslots = L.readers * PDT_INGEST_SLOTS;
    L.streams = c.streams;
    IngestSrc src;
    int fd = -1;
    if (c.source == SRC_MEM) src.mem = want.data();
    else {
        fd = pattern_file((size_t)c.off, c.bytes - c.missing, c.write_only ? O_WRONLY : O_RDONLY);
        src.fd = fd;
        src.off = c.off;
    }
    IngestJob J;
    // the direct-read arithmetic on an ordinary descriptor: reads start on the 4 KiB boundary below, `delta` is applied on copy
    if (c.source == SRC_FILE_DIRECT) J.fd_direct = dup(fd);
    J.mark_bytes = { 1, c.span, c.span + 1, c.bytes / 2, c.bytes, c.bytes + 12345 };
    std::vector<unsigned char> pin((size_t)L.nslots * L.slot_stride(J.fd_direct >= 0));
    J.arm(L, src, c.bytes, pin.data());
    CHECK(J.slot_stride == c.span + (c.source == SRC_FILE_DIRECT ? 8192 : 0));
    const size_t nmarks = J.mark_spans.size();
    CHECK(nmarks == 6 && J.mark_spans[0] == 1 && J.mark_spans[1] == 1 && J.mark_spans[2] == std::min<size_t>(2, L.nspans) && J.mark_spans[4] == L.nspans && J.mark_spans[5] == L.nspans);
    MemCopier C(&J, got.data(), c.fail_at);
    const bool background = c.background;
    auto submit = [&J, &C, background]() { IngestRing<MemCopier>{ J, C }.run(background); };
    CHECK(ingest_start(J, background, submit));
    int first_error = PDT_OK;
    if (background) {
        // a stream's waiter: prefix after prefix; a mark that is ready says all its spans have been queued
        for (size_t m = 0; m < nmarks; m++) {
            const int rc = J.wait_mark(m);
            if (rc == PDT_OK) {
                CHECK(first_error == PDT_OK);
                for (size_t k = 0; k < J.mark_spans[m]; k++) CHECK(J.submitted[k].load(std::memory_order_acquire) == 1);
            } else {
                CHECK(first_error == PDT_OK || rc == first_error);   // a later mark: the same error
                first_error = rc;
            }
        }
        CHECK(first_error == c.expect);
    } else if (!J.failed) {
        submit();
    }
    CHECK(J.join() == c.expect);
    CHECK(J.pool.empty() && J.wait_mark(nmarks) == PDT_ERR_STATE);
    if (c.expect != PDT_OK) {
        CHECK(J.wait_mark(nmarks - 1) == c.expect);                  // (returns: nothing will ever raise that mark)
        CHECK(c.fail_at < 0 || (int)C.order.size() == c.fail_at);
    } else {
        CHECK(C.order.size() == L.nspans);
        for (size_t m = 0; m < nmarks; m++) CHECK(J.wait_mark(m) == PDT_OK && C.mark_ok[m]);
        // no slot is left filled; the background form has waited for every copy, the foreground form leaves its last ones to
        // the stream that waits for them
        for (int s = 0; s < L.nslots; s++) {
            const int st = J.slot_state[(size_t)s].load();
            CHECK(st == 0 || (!background && st == 2 && C.slot[(size_t)s].on));
            CHECK((st == 2) == C.slot[(size_t)s].on);
        }
        C.finish();
        CHECK(memcmp(got.data(), want.data(), c.bytes) == 0);
    }
    if (fd >= 0) close(fd);
    alarm(0);
}

static void test_ring()
{
    const size_t span = 3000, bytes = 300 * span + 17;               // 301 spans, a short last one
    int n = 0;
    for (int background = 0; background < 2; background++)
        for (int source : { SRC_MEM, SRC_FILE, SRC_FILE_DIRECT })
            for (int readers : { 1, 3, 8 })
                for (int streams : { 1, 2, 4 }) {
                    RingCase c{ bytes, span, readers, streams, background != 0, source };
                    c.off = source == SRC_MEM ? 0 : 4099 + 44;      // not a multiple of 4096
                    run_ring(c);
                    n++;
                }
    // fewer spans than readers; a capture of one short span
    run_ring(RingCase{ 2 * span, span, 8, 4, true, SRC_MEM });
    run_ring(RingCase{ 5, span, 2, 1, false, SRC_FILE_DIRECT, 4095 });
    // wind-down
    for (int background = 0; background < 2; background++)
        for (int readers : { 1, 4 }) {
            for (int source : { SRC_FILE, SRC_FILE_DIRECT }) {
                RingCase c{ bytes, span, readers, 2, background != 0, source, 4099 };
                c.missing = 40 * span + 1;                           // the file ends early
                c.expect = PDT_ERR_FORMAT;
                run_ring(c);
                c.missing = 0;
                c.write_only = true;                                 // every read fails
                c.expect = PDT_ERR_IO;
                run_ring(c);
            }
            for (int fail_at : { 0, 1, 77, 300 }) {                  // the device refuses the n-th copy
                RingCase c{ bytes, span, readers, 3, background != 0, SRC_MEM };
                c.fail_at = fail_at;
                c.expect = PDT_ERR_NOGPU;
                run_ring(c);
            }
        }
    printf("ring: %d clean runs and the wind-down cases\n", n + 2);
}

int main(int argc, char **argv)
{
    g_dir = argc > 1 ? argv[1] : "/tmp";
    test_layout();
    test_cpulist();
    test_read_and_probe();
    test_ring();
    printf("ingest host: ok\n");
    return 0;
}
