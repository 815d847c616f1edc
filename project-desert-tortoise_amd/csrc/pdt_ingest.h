// pdt_ingest.h -- the host side of the host -> HBM ingest, free of HIP: how a capture is cut into spans (ingest_layout), how its
// file is probed and read (file_resident_fraction, read_fully, parse_cpulist), and the ring of pinned slots between the reader
// threads and the one thread that talks to the device (ingest_reader, IngestRing).  The ring is written over a copier type that
// supplies the four device operations; pdt_ingest.hip instantiates it with the HIP copier, tests/ingest_host_main.cc with a
// memcpy copier on a machine without a GPU.  Not installed, not part of the ABI.
#ifndef PDT_INGEST_H
#define PDT_INGEST_H
#include <errno.h>
#include <pthread.h>
#include <sched.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <sys/mman.h>
#include <unistd.h>

#include <algorithm>
#include <atomic>
#include <chrono>
#include <memory>
#include <thread>
#include <vector>

#include "../../include/pdt.h"

namespace pdtrt {

// The capture (a file the caller opened, or host memory) is cut into 2 MiB spans.  A few host threads bring the spans into
// pinned slots -- pread from the page cache resp. memcpy, ~5 GB/s per thread -- and one asynchronous copy per span is queued on a
// copy stream; a slot is refilled when its previous copy has completed.  The demodulation stream then waits for the last
// copy.  (One pageable hipMemcpy of the whole capture runs at a fraction of the link rate and cannot start before the file
// has been read.)  Small captures take the plain copy.
struct IngestSrc {
    const unsigned char *mem = nullptr;   // host memory, or
    int fd = -1;                          // an open file ...
    uint64_t off = 0;                     // ... and the byte offset of the first sample
};
constexpr size_t PDT_INGEST_SPAN_DEFAULT = 2u << 20;
constexpr int PDT_INGEST_SLOTS = 2;      // per thread
constexpr size_t PDT_INGEST_DIO = 4096;  // alignment of O_DIRECT reads (offset, length, address)

struct IngestLayout {
    size_t span = 0, nspans = 0;
    int readers = 0, nslots = 0, streams = 0;
    bool plain_copy = false;             // one hipMemcpyAsync on the demodulation stream, no threads
    // a direct read starts on the 4 KiB boundary below the span's first byte and ends on the one above its last
    size_t slot_stride(bool direct) const { return span + (direct ? 2 * PDT_INGEST_DIO : 0); }
    size_t mark_spans(size_t prefix_bytes) const { return std::min(nspans, (prefix_bytes + span - 1) / span); }
};
// `threads`, `span_mb`, `streams`: the tunings PDT_INGEST_THREADS / _SPAN_MB / _STREAMS (0 = not set); `hw`: hardware_concurrency
// (0 = unknown); `open_contexts`: contexts alive in this process
inline IngestLayout ingest_layout(size_t bytes, bool from_memory, bool has_job, int threads, int span_mb, int streams, unsigned hw, int open_contexts)
{
    IngestLayout L;
    // (hour-long captures: 8 MiB spans -- fewer, larger copies: 3.6 GB in 75-95 ms against 110 with 2 MiB spans)
    L.span = span_mb > 0 ? ((size_t)span_mb << 20) : (bytes >= ((size_t)512 << 20) ? 4 * PDT_INGEST_SPAN_DEFAULT : PDT_INGEST_SPAN_DEFAULT);
    L.nspans = (bytes + L.span - 1) / L.span;
    L.plain_copy = from_memory && L.nspans <= 2 && !has_job;
    // (round 4, 3.6 GB from tmpfs: 4 / 6 / 8 / 12 / 16 reader threads -> 100 / 92 / 88 / 90 / 89 ms for the whole call)
    // Several contexts of one process (bin/demodMulti: two per GPU) share the host's cores: half of them, divided by the open
    // contexts, never fewer than two readers (8 GPUs on a 256-thread host: 8 each; on a 32-thread host: 2 each).
    const unsigned share = std::max(2u, (hw ? hw / 2u : 8u) / (unsigned)std::max(1, open_contexts));
    const unsigned t_max = threads > 0 ? (unsigned)threads : std::min(8u, share);
    L.readers = std::max(1, (int)std::min<size_t>(std::min<unsigned>(hw ? hw / 2u + 1u : 4u, t_max), L.nspans));
    L.nslots = L.readers * PDT_INGEST_SLOTS;
    // copy streams in use: hour-long captures spread their span copies over four (3.6 GB: 123 -> 107 ms for the whole call,
    // ~51 GB/s from the page cache to HBM); ten-minute captures are no faster for it
    L.streams = std::min(4, std::max(1, streams > 0 ? streams : (bytes >= ((size_t)512 << 20) ? 4 : 1)));
    return L;
}

// ---- where a capture file's bytes are (round 6)
// Every byte of a capture crosses host memory three times on its way -- out of the page cache, into a pinned slot, out again by
// the DMA engine -- unless the file is read with O_DIRECT straight into the pinned slots: two.  At N = 8 GPUs the first is
// ~1.3 TB/s of host traffic against the ~1.0 - 1.1 the two sockets deliver.  O_DIRECT is right for a file that is NOT
// in the page cache (it then comes from the device either way; the copy through the cache is pure overhead) and wrong for one
// that is (tmpfs does not offer it at all): a probe of the file's pages decides.
constexpr int PDT_PROBE_SAMPLES = 64;
inline size_t probe_sample_page(int k, size_t npages) { return (size_t)(((double)k + 0.5) * (double)npages / PDT_PROBE_SAMPLES); }   // mid-interval
// fraction of the sampled pages that are in the page cache (1 = nothing to gain from O_DIRECT; also where it cannot be told)
inline double file_resident_fraction(int fd, uint64_t off, size_t bytes)
{
    const long page = sysconf(_SC_PAGESIZE);
    if (page <= 0 || bytes < (size_t)(64 * page)) return 1.0;
    const uint64_t a0 = off / (uint64_t)page * (uint64_t)page;
    const size_t len = (size_t)(off + bytes - a0);
    void *m = mmap(nullptr, len, PROT_READ, MAP_SHARED, fd, (off_t)a0);
    if (m == MAP_FAILED) return 1.0;
    const size_t npages = (len + (size_t)page - 1) / (size_t)page;
    int got = 0, res = 0;
    for (int k = 0; k < PDT_PROBE_SAMPLES; k++) {
        unsigned char vec = 0;
        if (mincore((unsigned char *)m + probe_sample_page(k, npages) * (size_t)page, (size_t)page, &vec) != 0) continue;
        got++;
        res += vec & 1;
    }
    munmap(m, len);
    return got ? (double)res / (double)got : 1.0;
}

// a kernel cpulist ("0-3,8,10-11\n") into a CPU set; false where it names no CPU (below CPU_SETSIZE)
inline bool parse_cpulist(const char *text, cpu_set_t *set)
{
    CPU_ZERO(set);
    bool any = false;
    for (const char *p = text;;) {
        char *end = nullptr;
        const long a = strtol(p, &end, 10);
        if (end == p || a < 0) break;
        long b = a;
        if (*end == '-') {
            p = end + 1;
            b = strtol(p, &end, 10);
            if (end == p) break;
        }
        for (long c = a; c <= b && c < CPU_SETSIZE; c++) { CPU_SET((int)c, set); any = true; }
        if (*end != ',') break;
        p = end + 1;
    }
    return any;
}

// what stopped an ingest (IngestJob::failed)
enum { INGEST_DEVICE = 1, INGEST_SHORT = 2, INGEST_READ = 3 };
inline int ingest_error(int failed)
{
    if (!failed) return PDT_OK;
    if (failed == INGEST_SHORT) return PDT_ERR_FORMAT;                // the file is shorter than announced
    return failed == INGEST_READ ? PDT_ERR_IO : PDT_ERR_NOGPU;
}

// pread, at most `want` bytes, until at least `need` have arrived: 0, INGEST_SHORT (the file ends early) or INGEST_READ
inline int read_fully(int fd, unsigned char *buf, size_t want, size_t need, uint64_t offset)
{
    for (size_t got = 0; got < need;) {
        const ssize_t r = pread(fd, buf + got, want - got, (off_t)(offset + got));
        if (r < 0 && errno == EINTR) continue;
        if (r <= 0) return r == 0 ? INGEST_SHORT : INGEST_READ;
        got += (size_t)r;
    }
    return 0;
}

// One ingest: what its threads share.  In the background form (a job of the caller's) every span has a flag that says its copy
// has been queued; the caller makes its stream wait for the spans of a prefix (ingest_wait_mark) and starts work on it while
// the rest still arrives, and joins the threads at the end (ingest_join).
struct IngestJob {
    std::vector<std::thread> pool;
    std::unique_ptr<std::atomic<int>[]> submitted;
    std::unique_ptr<std::atomic<int>[]> slot_state;                  // 0 free, 1 filled (to be copied), 2 copy in flight
    std::unique_ptr<size_t[]> slot_span;                             // the span a filled slot holds (written before state 1)
    std::unique_ptr<size_t[]> slot_delta;                            // ... and where in the slot its first byte lies (O_DIRECT reads start on a 4 KiB boundary of the file)
    int fd_direct = -1;                                              // the capture file once more, opened with O_DIRECT (or -1)
    ~IngestJob() { if (fd_direct >= 0) close(fd_direct); }
    std::atomic<int> failed{0};
    IngestLayout lay;
    IngestSrc src;
    size_t bytes = 0, slot_stride = 0;
    unsigned char *pin = nullptr;                                    // lay.nslots slots of slot_stride bytes
    bool have_cpus = false, debug = false;                           // the readers run on `cpus`; PDT_DEBUG_OVERLAP
    cpu_set_t cpus;
    // prefixes the caller will wait for (bytes, ascending; set before ingest_capture): when the last span of prefix m has been
    // queued the submitter records mark m -- behind that prefix's copies and in front of everything later -- and raises mark_ready[m]
    std::vector<size_t> mark_bytes;
    std::vector<size_t> mark_spans;
    std::unique_ptr<std::atomic<int>[]> mark_ready;

    // (fd_direct is set before: it decides the slots' stride)
    void arm(const IngestLayout &layout, const IngestSrc &source, size_t nbytes, unsigned char *pinned)
    {
        lay = layout;
        src = source;
        bytes = nbytes;
        pin = pinned;
        slot_stride = lay.slot_stride(fd_direct >= 0);
        failed = 0;
        submitted.reset(new std::atomic<int>[lay.nspans]);
        for (size_t k = 0; k < lay.nspans; k++) submitted[k].store(0);
        slot_state.reset(new std::atomic<int>[(size_t)lay.nslots]);
        slot_span.reset(new size_t[(size_t)lay.nslots]);
        slot_delta.reset(new size_t[(size_t)lay.nslots]);
        for (int q = 0; q < lay.nslots; q++) { slot_state[(size_t)q].store(0); slot_delta[(size_t)q] = 0; }
        mark_spans.clear();
        for (size_t b : mark_bytes) mark_spans.push_back(lay.mark_spans(b));
        mark_ready.reset(new std::atomic<int>[mark_spans.size() + 1]);
        for (size_t m = 0; m < mark_spans.size(); m++) mark_ready[m].store(0);
    }
    // the host's part of ingest_wait_mark: until mark m has been recorded, or the ingest has failed
    int wait_mark(size_t m)
    {
        if (m >= mark_spans.size()) return PDT_ERR_STATE;
        while (!mark_ready[m].load(std::memory_order_acquire)) {
            if (failed) return ingest_error(failed);
            std::this_thread::sleep_for(std::chrono::microseconds(20));
        }
        return PDT_OK;
    }
    int join()
    {
        for (auto &th : pool) th.join();
        pool.clear();
        return ingest_error(failed);
    }
};

// span k is read by thread k % T into its slot (k / T) % SLOTS: slot index (k % T) * SLOTS + (k / T) % SLOTS
inline void ingest_reader(IngestJob *J, int t)
{
    std::atomic<int> &failed = J->failed;
    const IngestLayout &L = J->lay;
    const IngestSrc &src = J->src;
    if (J->have_cpus) (void)pthread_setaffinity_np(pthread_self(), sizeof J->cpus, &J->cpus);      // the GPU's socket
    int round = 0;
    for (size_t k = (size_t)t; k < L.nspans && !failed; k += (size_t)L.readers, round++) {
        const int slot = t * PDT_INGEST_SLOTS + (round % PDT_INGEST_SLOTS);
        std::atomic<int> &st = J->slot_state[(size_t)slot];
        while (st.load(std::memory_order_acquire) != 0) {          // its previous copy is still on its way
            if (failed) return;
            std::this_thread::sleep_for(std::chrono::microseconds(10));
        }
        unsigned char *pin = J->pin + (size_t)slot * J->slot_stride;
        const size_t at = k * L.span;
        const size_t len = std::min(L.span, J->bytes - at);
        size_t delta = 0;
        if (src.mem) {
            memcpy(pin, src.mem + at, len);
        } else {
            // direct: from the device straight into the pinned slot: the read starts on the 4 KiB boundary below the span's first
            // byte and ends on the one above its last (the slot has the room), the copy to the GPU starts `delta` bytes in
            const bool direct = J->fd_direct >= 0;
            const uint64_t fo = src.off + at;
            if (direct) delta = (size_t)(fo & (PDT_INGEST_DIO - 1));
            const size_t want = direct ? (delta + len + PDT_INGEST_DIO - 1) & ~(PDT_INGEST_DIO - 1) : len;
            if (const int f = read_fully(direct ? J->fd_direct : src.fd, pin, want, delta + len, fo - delta)) { failed = f; return; }
        }
        J->slot_span[(size_t)slot] = k;
        J->slot_delta[(size_t)slot] = delta;
        st.store(1, std::memory_order_release);
    }
}

// Round 5: ONE thread talks to the device.  The readers only fill pinned slots (pread / memcpy) and raise a flag; the
// submitter -- the calling thread, or one more background thread when the ingest runs beside the chain -- queues the copies
// and hands a slot back to its reader when its copy has completed (the oldest copy in flight of each copy stream is polled).
// With eight readers calling hipMemcpyAsync / hipEventRecord / hipEventSynchronize themselves the runtime's locks were
// contended: beside a chain that is launching kernels the ingest fell from 52 to ~41 GB/s, and a burst of fifty launches took
// up to 7 ms instead of 0.2 (round 4: "the readers contend with the launches in the runtime").
// A Copier has
//   bool set_device();
//   bool queue(int slot, int q, size_t at, const unsigned char *from, size_t len);   // copy stream q: from -> capture byte `at`
//   int done(int slot, bool block);     // the slot's last copy: 1 completed, 0 not yet (never with block), < 0 failed
//   bool mark(size_t m);                // on every copy stream: behind what has been queued, in front of what will be
template <class Copier> struct IngestRing {
    IngestJob &J;
    Copier &C;
    // Spans are queued as their slots fill, in whatever order that is: a reader that is late (descheduled: the hosts are
    // shared) holds up its own two slots only, not the ring (queued strictly in span order, one late reader stopped all
    // copies).  `upto` = every span below it has been queued: what the prefixes' marks go by.  Per copy stream the slots in
    // flight form a queue, oldest first.
    std::vector<int> inflight[4];
    size_t head[4] = { 0, 0, 0, 0 };
    size_t upto = 0, queued = 0, mi = 0;
    int rr = 0;                                                    // copy streams round robin

    void retire(bool block)
    {
        for (int q = 0; q < J.lay.streams; q++)
            while (head[q] < inflight[q].size()) {
                const int slot = inflight[q][head[q]];
                const int e = C.done(slot, block);
                if (e == 0) break;
                if (e < 0) { J.failed = INGEST_DEVICE; return; }
                J.slot_state[(size_t)slot].store(0, std::memory_order_release);
                head[q]++;
            }
    }
    void marks()                                                   // prefixes complete with the spans queued so far
    {
        while (upto < J.lay.nspans && J.submitted[upto].load(std::memory_order_relaxed)) upto++;
        while (mi < J.mark_spans.size() && J.mark_spans[mi] <= upto) {
            if (!C.mark(mi)) { J.failed = INGEST_DEVICE; return; }
            J.mark_ready[mi].store(1, std::memory_order_release);
            mi++;
        }
    }
    int queue_filled()                                             // every filled slot: 1, 0 = none was, < 0 = the device refused
    {
        int any = 0;
        for (int slot = 0; slot < J.lay.nslots && !J.failed; slot++) {
            if (J.slot_state[(size_t)slot].load(std::memory_order_acquire) != 1) continue;
            const size_t k = J.slot_span[(size_t)slot];
            const size_t at = k * J.lay.span;
            const int q = rr;
            rr = (rr + 1 == J.lay.streams) ? 0 : rr + 1;
            if (!C.queue(slot, q, at, J.pin + (size_t)slot * J.slot_stride + J.slot_delta[(size_t)slot], std::min(J.lay.span, J.bytes - at))) {
                J.failed = INGEST_DEVICE;
                return -1;
            }
            J.slot_state[(size_t)slot].store(2, std::memory_order_release);
            inflight[q].push_back(slot);
            J.submitted[k].store(1, std::memory_order_release);
            queued++;
            any = 1;
            marks();
        }
        return any;
    }
    void run(bool background)
    {
        std::atomic<int> &failed = J.failed;
        if (!C.set_device()) { failed = INGEST_DEVICE; return; }
        // (developer aid, PDT_DEBUG_OVERLAP: how long the submitter had nothing to queue, and how many copies were in flight on
        // average while it waited -- near the ring's half: the copies are the pace (a reader refills a slot as soon as its copy has
        // completed); near zero: the readers are)
        double idle_ms = 0, flying_sum = 0, api_ms = 0;
        long long idle_n = 0;
        const auto t_sub0 = std::chrono::steady_clock::now();
        while (queued < J.lay.nspans && !failed) {
            const auto t_it0 = std::chrono::steady_clock::now();
            const int any = queue_filled();
            if (any < 0) return;
            retire(false);
            const auto t_it1 = std::chrono::steady_clock::now();
            api_ms += std::chrono::duration<double, std::milli>(t_it1 - t_it0).count();
            if (!any) {
                int flying = 0;
                for (int slot = 0; slot < J.lay.nslots; slot++) flying += J.slot_state[(size_t)slot].load(std::memory_order_relaxed) == 2;
                std::this_thread::sleep_for(std::chrono::microseconds(15));
                idle_ms += std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t_it1).count();
                flying_sum += flying;
                idle_n++;
            }
        }
        marks();
        if (J.debug)
            fprintf(stderr, "ingest submitter: %.2f ms in all: %.2f in the runtime (queueing, polling), %.2f with nothing to queue (%.1f of %d slots in flight on average)\n",
                    std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t_sub0).count(), api_ms, idle_ms,
                    idle_n ? flying_sum / (double)idle_n : 0.0, J.lay.nslots);
        // the background form leaves the pinned slots free; the foreground form returns with its last copies still on their way
        // (the caller's stream waits for them, and the call does not return before that stream is idle)
        if (background) retire(true);
    }
};

// the readers and, in the background form, one more thread for `submit`; false: a thread could not be started
template <class Submit> bool ingest_start(IngestJob &J, bool background, Submit submit)
{
    try {
        for (int t = 0; t < J.lay.readers; t++) J.pool.emplace_back(ingest_reader, &J, t);
        if (background) J.pool.emplace_back(submit);
    } catch (const std::exception &) {
        J.failed = INGEST_DEVICE;
        return false;
    }
    return true;
}

}  // namespace pdtrt
#endif
