// pdt_ingest.hip -- the device side of the host -> HBM ingest (the host side, with the ring of pinned slots: pdt_ingest.h): a
// context's pinned staging, copy streams and events (IngestRes), the copier the ring runs over, and ingest_capture /
// ingest_wait_mark / ingest_join.  No kernels.
#include "pdt_rt.h"

#include <sys/syscall.h>

namespace {

std::atomic<int> g_open_contexts{0};          // contexts alive in this process (pdt_open / pdt_close)
// One ingest per GPU at a time.  Two contexts on one GPU (bin/demodMulti's two lanes) that read their captures at once would
// share the PCIe link and both arrive late; taking turns, the second one's capture arrives while the first one's chain runs.
std::mutex g_link_mu[64];

// the NUMA node a GPU hangs on, and that node's CPUs
int gpu_numa_node(int device)
{
    char bus[64] = {0}, path[160];
    if (hipDeviceGetPCIBusId(bus, (int)sizeof bus, device) != hipSuccess) { (void)hipGetLastError(); return -1; }
    for (char *c = bus; *c; c++) *c = (char)tolower((unsigned char)*c);
    snprintf(path, sizeof path, "/sys/bus/pci/devices/%s/numa_node", bus);
    FILE *f = fopen(path, "r");
    int node = -1;
    if (f) { if (fscanf(f, "%d", &node) != 1) node = -1; fclose(f); }
    return node;
}
bool node_cpus(int node, cpu_set_t *set)
{
    char path[96], text[4096] = {0};
    snprintf(path, sizeof path, "/sys/devices/system/node/node%d/cpulist", node);
    FILE *f = fopen(path, "r");
    if (!f) return false;
    const size_t n = fread(text, 1, sizeof text - 1, f);
    fclose(f);
    return n > 0 && parse_cpulist(text, set);
}

// How the file is read: O_DIRECT straight into the pinned slots when its pages are not cached (file_resident_fraction) -- the
// descriptor goes to the job --, and the NUMA node readers and staging are bound to (-1: none).
int read_mode(const pdt_ctx *ctx, const IngestSrc &src, size_t bytes, IngestJob *J)
{
    if (J->fd_direct >= 0) close(J->fd_direct);
    J->fd_direct = -1;
    if (src.mem || bytes < ((size_t)64 << 20)) return -1;
    const int direct = ctx->tune.ingest_direct, numa = ctx->tune.ingest_numa;
    if (direct > 0 || (direct < 0 && file_resident_fraction(src.fd, src.off, bytes) < 0.1)) {
        char link[64];
        snprintf(link, sizeof link, "/proc/self/fd/%d", src.fd);
        J->fd_direct = open(link, O_RDONLY | O_DIRECT | O_CLOEXEC);        // (EINVAL where the file system has no direct I/O: tmpfs)
    }
    const int gnode = gpu_numa_node(ctx->cfg.device);
    // (Measured, round 6, one box -- GPU and the capture's pages both on node 1: readers and staging bound there 100 - 106 ms for
    // the 3.6 GB file -> frame file path, not bound 94.6, profiles/r6/e2e_ab_numa.txt: eight readers crowd one socket's cores
    // beside the box's other tenants, as in round 4.  So buffered reads are bound on request only (PDT_INGEST_NUMA); direct
    // reads -- the device writes the staging memory, the GPU's DMA engine reads it -- keep staging and readers on the GPU's node.)
    return gnode >= 0 && (numa > 0 || (numa < 0 && J->fd_direct >= 0)) ? gnode : -1;
}

// The copy streams live at the LOWEST stream priority: streams of one priority share a few hardware queues, and a copy stream
// that lands on the queue of the demodulation stream waits behind that stream's kernels -- beside a running segment (a 5 ms PLL
// kernel) one of four copy streams stood still, and with it the ring of pinned slots: the overlapped ingest crawled at
// ~25 GB/s while kernels ran (round 5, tools/jobs/r5_e2e_ab.sh: four streams 95 ms, two -- no sharing -- 82 ms).  Another
// priority is another set of queues (the side stream uses the highest for the same reason).
hipError_t make_copy_stream(hipStream_t *out)
{
    int least = 0, greatest = 0;
    (void)hipDeviceGetStreamPriorityRange(&least, &greatest);
    if (least != greatest && hipStreamCreateWithPriority(out, hipStreamNonBlocking, least) == hipSuccess) return hipSuccess;
    (void)hipGetLastError();
    return hipStreamCreateWithFlags(out, hipStreamNonBlocking);
}
int grow_events(std::vector<hipEvent_t> &ev, size_t n)
{
    while (ev.size() < n) {
        hipEvent_t e;
        HIP_TRY(hipEventCreateWithFlags(&e, hipEventDisableTiming));
        ev.push_back(e);
    }
    return PDT_OK;
}
// (A context's first ingest sets these up, and a one-shot process -- bin/demodPOES -- pays for it in full: a stream is ~10 ms
// to create, its first copy ~6 ms more (the runtime starts its DMA queue then), the pinned staging 25 - 30 ms:
// tools/probes/cold_path_probe.hip.  Setting them up side by side, a thread each, was measured and made it WORSE -- the pinned
// allocation alone then took 0.1 - 0.7 s: the runtime serialises them, badly.  One after the other.)
int prepare_resources(pdt_ctx *ctx, const IngestLayout &lay, size_t need, int bind_node, size_t nmarks)
{
    IngestRes &R = ctx->ingest;
    const auto t_setup0 = std::chrono::steady_clock::now();
    if (need > R.pin_cap) {
        if (R.pin) (void)hipHostFree(R.pin);
        R.pin = nullptr;
        R.pin_cap = 0;
        // (the staging memory on the node the readers run on: MPOL_PREFERRED = 1 for this thread while the runtime allocates and
        // pins it, MPOL_DEFAULT = 0 again afterwards)
        unsigned long mask[16] = {0};
        if (bind_node >= 0 && bind_node < 1024) {
            mask[bind_node / (8 * sizeof(long))] = 1ul << (bind_node % (8 * sizeof(long)));
            (void)syscall(SYS_set_mempolicy, 1, mask, (unsigned long)(8 * sizeof mask));
        }
        const hipError_t he = timed_host_malloc(&R.pin, need);
        if (bind_node >= 0) (void)syscall(SYS_set_mempolicy, 0, nullptr, 0ul);
        if (he != hipSuccess) { (void)hipGetLastError(); return PDT_ERR_NOMEM; }
        R.pin_cap = need;
    }
    for (int q = 0; q < lay.streams; q++) {
        if (!R.copy[q]) HIP_TRY(make_copy_stream(&R.copy[q]));
        if (!R.all_queued[q]) HIP_TRY(hipEventCreateWithFlags(&R.all_queued[q], hipEventDisableTiming));
    }
    int rc;
    if ((rc = grow_events(R.slot_ev, (size_t)lay.nslots)) || (rc = grow_events(R.mark_ev, nmarks * (size_t)lay.streams))) return rc;
    // the destination may still be read by work queued earlier on the demodulation stream (all_queued[0] is free until the end)
    HIP_TRY(hipEventRecord(R.all_queued[0], ctx->stream));
    for (int q = 0; q < lay.streams; q++) HIP_TRY(hipStreamWaitEvent(R.copy[q], R.all_queued[0], 0));
    if (ctx->tune.debug_overlap)
        fprintf(stderr, "ingest_capture: streams / events / pinned staging ready after %.2f ms\n",
                std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t_setup0).count());
    return PDT_OK;
}

// the ring's four device operations (pdt_ingest.h): one event per slot behind its copy, one per mark and copy stream
struct HipCopier {
    IngestRes *R;
    unsigned char *dst;
    int device, streams;
    bool set_device() { return hipSetDevice(device) == hipSuccess; }
    bool queue(int slot, int q, size_t at, const unsigned char *from, size_t len)
    {
        return hipMemcpyAsync(dst + at, from, len, hipMemcpyHostToDevice, R->copy[q]) == hipSuccess &&
               hipEventRecord(R->slot_ev[(size_t)slot], R->copy[q]) == hipSuccess;
    }
    int done(int slot, bool block)
    {
        const hipError_t e = block ? hipEventSynchronize(R->slot_ev[(size_t)slot]) : hipEventQuery(R->slot_ev[(size_t)slot]);
        if (e == hipErrorNotReady) { (void)hipGetLastError(); return 0; }
        return e == hipSuccess ? 1 : -1;
    }
    bool mark(size_t m)
    {
        for (int q = 0; q < streams; q++)
            if (hipEventRecord(R->mark_ev[m * (size_t)streams + (size_t)q], R->copy[q]) != hipSuccess) return false;
        return true;
    }
};

}  // namespace

void IngestRes::release()
{
    if (pin) (void)hipHostFree(pin);
    for (hipEvent_t e : slot_ev) (void)hipEventDestroy(e);
    for (hipEvent_t e : mark_ev) (void)hipEventDestroy(e);
    for (int q = 0; q < 4; q++) {
        if (all_queued[q]) (void)hipEventDestroy(all_queued[q]);
        if (copy[q]) (void)hipStreamDestroy(copy[q]);
    }
    *this = IngestRes();
}

namespace pdtrt {

std::atomic<int> &ingest_open_contexts() { return g_open_contexts; }
std::mutex &ingest_link(int device) { return g_link_mu[(unsigned)device % 64u]; }

int ingest_capture(pdt_ctx *ctx, const IngestSrc &src, size_t bytes, void *dst, IngestJob *job)
{
    IngestRes &R = ctx->ingest;
    R.was_direct = 0;
    R.numa_node = -1;
    if (!bytes) return PDT_OK;
    const Tuning &tu = ctx->tune;
    const IngestLayout lay = ingest_layout(bytes, src.mem != nullptr, job != nullptr, tu.ingest_threads, tu.ingest_span_mb, tu.ingest_streams,
                                           std::thread::hardware_concurrency(), g_open_contexts.load());
    if (lay.plain_copy) {
        HIP_TRY(hipMemcpyAsync(dst, src.mem, bytes, hipMemcpyHostToDevice, ctx->stream));
        return PDT_OK;
    }
    IngestJob local;
    IngestJob *J = job ? job : &local;
    const int bind_node = read_mode(ctx, src, bytes, J);
    R.was_direct = J->fd_direct >= 0 ? 1 : 0;
    R.numa_node = bind_node;
    int rc = prepare_resources(ctx, lay, (size_t)lay.nslots * lay.slot_stride(J->fd_direct >= 0), bind_node, J->mark_bytes.size());
    if (rc) return rc;
    J->arm(lay, src, bytes, (unsigned char *)R.pin);
    J->have_cpus = bind_node >= 0 && node_cpus(bind_node, &J->cpus);
    J->debug = tu.debug_overlap;
    const bool background = job != nullptr;
    const HipCopier copier{ &R, (unsigned char *)dst, ctx->cfg.device, lay.streams };
    auto submit = [J, copier, background]() {
        std::lock_guard<std::mutex> link(ingest_link(copier.device));      // (the readers fill their first slots meanwhile)
        HipCopier C = copier;
        IngestRing<HipCopier>{ *J, C }.run(background);
    };
    const bool started = ingest_start(*J, background, submit);
    // (background form: the readers are already running and may have set `failed` -- a short file, a read error: those codes
    // come through ingest_wait_mark / ingest_join, always; only a thread that could not be started is reported here)
    if (background) return started ? PDT_OK : PDT_ERR_NOMEM;           // (the caller joins: ingest_join)
    if (!J->failed) submit();
    if ((rc = ingest_join(*J))) return rc;
    for (int q = 0; q < lay.streams; q++) {
        HIP_TRY(hipEventRecord(R.all_queued[q], R.copy[q]));
        HIP_TRY(hipStreamWaitEvent(ctx->stream, R.all_queued[q], 0));
    }
    return PDT_OK;
}

// make `stream` wait for the copies of prefix `m` of the job (IngestJob::mark_bytes).  The host waits -- without touching the HIP
// runtime: the submitter is in it all the time -- until the submitter has queued the prefix's last span and recorded one event
// per copy stream behind it; the stream then waits for those events: for the prefix's copies and for nothing that was queued
// later.  (Round 3 recorded an event per span and made the stream wait for each: ~300 calls, and the host's loop lagged 10 ms
// behind the data.)
int ingest_wait_mark(pdt_ctx *ctx, IngestJob &job, size_t m, hipStream_t stream)
{
    if (const int rc = job.wait_mark(m)) return rc;
    for (int q = 0; q < job.lay.streams; q++) HIP_TRY(hipStreamWaitEvent(stream, ctx->ingest.mark_ev[m * (size_t)job.lay.streams + (size_t)q], 0));
    return PDT_OK;
}

int ingest_join(IngestJob &job)
{
    const int rc = job.join();
    if (rc == PDT_ERR_NOGPU) (void)hipGetLastError();
    return rc;
}

}  // namespace pdtrt
