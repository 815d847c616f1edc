// pdt_tip_subcom.hip -- decommutation of TIP minor frames: subcommutated bytes by table (pdt_tip_subcom.h): the kernels k_subcom_mark,
// k_subcom_count, k_subcom_scan, k_subcom_place and k_subcom_spikes, their launch, the host restatement pdt_host_tip_subcom, the
// built-in tables and the samples' text.  A unit of its own, beside pdt_tip_dcs.hip.
#include <hip/hip_runtime.h>
#include <errno.h>
#include <unistd.h>
#include <algorithm>
#include <exception>
#include <string>
#include <vector>

#include "../../include/pdt.h"
#include "pdt_tip_subcom.h"

static_assert(sizeof(pdt_frame) == sizeof(pdt::TipDcsRec) && sizeof(pdt_frame) == 136, "pdt_frame");
static_assert(sizeof(pdt_subcom_entry) == sizeof(pdt::TipSubcomEntry) && sizeof(pdt_subcom_entry) == 10, "pdt_subcom_entry");
static_assert(offsetof(pdt_subcom_entry, channel) == offsetof(pdt::TipSubcomEntry, channel) && offsetof(pdt_subcom_entry, byte) == offsetof(pdt::TipSubcomEntry, byte) &&
              offsetof(pdt_subcom_entry, period) == offsetof(pdt::TipSubcomEntry, period) && offsetof(pdt_subcom_entry, phase) == offsetof(pdt::TipSubcomEntry, phase) &&
              offsetof(pdt_subcom_entry, mask) == offsetof(pdt::TipSubcomEntry, mask) && offsetof(pdt_subcom_entry, shift) == offsetof(pdt::TipSubcomEntry, shift) &&
              offsetof(pdt_subcom_entry, invert) == offsetof(pdt::TipSubcomEntry, invert), "pdt_subcom_entry");
static_assert(sizeof(pdt_subcom_sample) == sizeof(pdt::TipSubcomSample) && sizeof(pdt_subcom_sample) == 24, "pdt_subcom_sample");
static_assert(offsetof(pdt_subcom_sample, frame) == offsetof(pdt::TipSubcomSample, frame) && offsetof(pdt_subcom_sample, minor_id) == offsetof(pdt::TipSubcomSample, minor_id) &&
              offsetof(pdt_subcom_sample, channel) == offsetof(pdt::TipSubcomSample, channel) && offsetof(pdt_subcom_sample, entry) == offsetof(pdt::TipSubcomSample, entry) &&
              offsetof(pdt_subcom_sample, value) == offsetof(pdt::TipSubcomSample, value) && offsetof(pdt_subcom_sample, raw) == offsetof(pdt::TipSubcomSample, raw) &&
              offsetof(pdt_subcom_sample, flags) == offsetof(pdt::TipSubcomSample, flags) && offsetof(pdt_subcom_sample, flags) == 18, "pdt_subcom_sample");
static_assert(sizeof(pdt_subcom_summary) == sizeof(pdt::TipSubcomSummary) && sizeof(pdt_subcom_summary) == 72, "pdt_subcom_summary");
static_assert(sizeof(pdt_subcom_cfg) == 8, "pdt_subcom_cfg");
static_assert(PDT_SUBCOM_BYTE_PARITY == pdt::TIP_SUBCOM_BYTE_PARITY && PDT_SUBCOM_ID_PARITY == pdt::TIP_SUBCOM_ID_PARITY &&
              PDT_SUBCOM_UNCOVERED == pdt::TIP_SUBCOM_UNCOVERED && PDT_SUBCOM_SPIKE == pdt::TIP_SUBCOM_SPIKE, "flags");
static_assert(PDT_SUBCOM_SEM == pdt::TIP_SUBCOM_SEM && PDT_SUBCOM_HK == pdt::TIP_SUBCOM_HK, "tables");

namespace pdt {

// Where the records are: the caller's pdt_frame records, or the chain's own (no time stamp: the stamps come up from the host beside
// them).  Strides and offsets in bytes; the flags are nbytes and, behind it, complete.
struct SubcomSrc {
    const unsigned char *recs, *times;
    unsigned stride, tstride, o_nbytes, o_bytes;
};

// the counters on the device (SubcomWork's first region)
enum { SUBCOM_C_USED = 0, SUBCOM_C_SKIPPED, SUBCOM_C_BAD_ID, SUBCOM_C_SAMPLES, SUBCOM_C_DROPPED, SUBCOM_C_BYTE_PARITY, SUBCOM_C_ID_PARITY, SUBCOM_C_SPIKES,
       SUBCOM_C_HIT, SUBCOM_C_COUNT };

// the table, and the rule's switches, as every kernel takes them
struct SubcomRule {
    const TipSubcomEntry *table;
    int ne, nchan, trusted_only, thr;
};

// Stage 1, a lane per record: eligibility, the counter, the five groups' parity and bad_id, in one word (tip_subcom_mark).
__global__ void __launch_bounds__(256) k_subcom_mark(SubcomSrc S, unsigned long long n, unsigned *__restrict__ marks)
{
    const unsigned long long i = (unsigned long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const unsigned char *r = S.recs + i * S.stride;
    marks[i] = tip_subcom_mark(r[S.o_nbytes + 1], r[S.o_nbytes], r + S.o_bytes);
}

__device__ __forceinline__ void subcom_load_table(TipSubcomEntry *s_tab, const SubcomRule &R)
{
    for (int k = (int)threadIdx.x; k < R.ne; k += (int)blockDim.x) s_tab[k] = R.table[k];
}

// does entry E leave a sample in the record whose mark is m?  *fl: its flags; *dropped: it fired and trusted_only took it
__device__ __forceinline__ bool subcom_exists(const TipSubcomEntry &E, unsigned m, int trusted_only, unsigned *fl, bool *dropped)
{
    *dropped = false;
    *fl = 0;
    if (!(m & TIP_SUBCOM_M_USED) || !tip_subcom_fires(E, tip_subcom_mark_id(m))) return false;
    *fl = tip_subcom_flags(E.byte, tip_subcom_mark_failed(m));
    *dropped = trusted_only && tip_subcom_untrusted(*fl);
    return !*dropped;
}

// Stage 2, a wavefront per tile of 64 records, lane = record: per entry the ballot of "leaves a sample here" is the entry's count in
// the tile; the counts go to the entry's channel.  cnt[channel * tiles + tile].  The tile's summary counters go by atomics.
__global__ void __launch_bounds__(TIP_SUBCOM_TILE) k_subcom_count(SubcomRule R, unsigned long long n, unsigned long long tiles, const unsigned *__restrict__ marks,
                                                                  unsigned *__restrict__ cnt, unsigned long long *__restrict__ sum)
{
    __shared__ TipSubcomEntry s_tab[TIP_SUBCOM_MAX_ENTRIES];
    __shared__ unsigned s_cnt[TIP_SUBCOM_MAX_CHANNELS];
    const unsigned long long tile = blockIdx.x, i = tile * TIP_SUBCOM_TILE + threadIdx.x;
    const int lane = (int)threadIdx.x;
    subcom_load_table(s_tab, R);
    for (int c = lane; c < R.nchan; c += TIP_SUBCOM_TILE) s_cnt[c] = 0;
    __syncthreads();
    const unsigned m = i < n ? marks[i] : 0u;
    const unsigned inside = (unsigned)__popcll(__ballot(i < n)), used = (unsigned)__popcll(__ballot(m & TIP_SUBCOM_M_USED)),
                   bad = (unsigned)__popcll(__ballot(m & TIP_SUBCOM_M_BAD_ID));
    unsigned dropped = 0, byte_parity = 0, id_parity = 0;
    if (used)
        for (int e = 0; e < R.ne; e++) {
            const TipSubcomEntry E = s_tab[e];
            unsigned fl;
            bool drop;
            const bool ex = subcom_exists(E, m, R.trusted_only, &fl, &drop);
            const unsigned long long bx = __ballot(ex), bd = __ballot(drop);
            if (!(bx | bd)) continue;
            const unsigned c = (unsigned)__popcll(bx);
            dropped += (unsigned)__popcll(bd);
            byte_parity += (unsigned)__popcll(__ballot(ex && (fl & TIP_SUBCOM_BYTE_PARITY)));
            id_parity += (unsigned)__popcll(__ballot(ex && (fl & TIP_SUBCOM_ID_PARITY)));
            if (lane == 0) s_cnt[E.channel] += c;
        }
    __syncthreads();
    for (int c = lane; c < R.nchan; c += TIP_SUBCOM_TILE) cnt[(unsigned long long)c * tiles + tile] = s_cnt[c];
    if (lane == 0) {
        if (used) atomicAdd(&sum[SUBCOM_C_USED], (unsigned long long)used);
        if (bad) atomicAdd(&sum[SUBCOM_C_BAD_ID], (unsigned long long)bad);
        if (inside - used - bad) atomicAdd(&sum[SUBCOM_C_SKIPPED], (unsigned long long)(inside - used - bad));
        if (dropped) atomicAdd(&sum[SUBCOM_C_DROPPED], (unsigned long long)dropped);
        if (byte_parity) atomicAdd(&sum[SUBCOM_C_BYTE_PARITY], (unsigned long long)byte_parity);
        if (id_parity) atomicAdd(&sum[SUBCOM_C_ID_PARITY], (unsigned long long)id_parity);
    }
}

// Stage 3, one workgroup of four wavefronts: a wavefront takes a channel at a time and scans its tiles' counts, 64 at a step, into each
// tile's place within the channel (in place); then one thread scans the channels' totals into offsets[0 .. nchan].  The sample count
// stays here, in the counters and in offsets[nchan].
constexpr int SUBCOM_SCAN_THREADS = 256;
__global__ void __launch_bounds__(SUBCOM_SCAN_THREADS) k_subcom_scan(int nchan, unsigned long long tiles, unsigned *__restrict__ cnt,
                                                                     unsigned long long *__restrict__ offsets, unsigned long long *__restrict__ sum)
{
    __shared__ unsigned s_total[TIP_SUBCOM_MAX_CHANNELS];
    const int lane = (int)(threadIdx.x & 63), wave = (int)(threadIdx.x >> 6);
    for (int c = wave; c < nchan; c += SUBCOM_SCAN_THREADS / 64) {
        unsigned *row = cnt + (unsigned long long)c * tiles;
        unsigned carry = 0;
        for (unsigned long long t0 = 0; t0 < tiles; t0 += 64) {
            const unsigned long long k = t0 + lane;
            const unsigned v = k < tiles ? row[k] : 0u;
            unsigned incl = v;
#pragma unroll
            for (int d = 1; d < 64; d <<= 1) {
                const unsigned o = __shfl_up(incl, d);
                if (lane >= d) incl += o;
            }
            if (k < tiles) row[k] = carry + incl - v;
            carry += __shfl(incl, 63);
        }
        if (lane == 0) s_total[c] = carry;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        unsigned long long run = 0, hit = 0;
        for (int c = 0; c < nchan; c++) {
            offsets[c] = run;
            run += s_total[c];
            hit += s_total[c] != 0;
        }
        offsets[nchan] = run;
        sum[SUBCOM_C_SAMPLES] = run;
        sum[SUBCOM_C_HIT] = hit;
    }
}

// Stage 4, a wavefront per tile, lane = record.  A sample's place is offsets[channel] + the tile's place in the channel + its rank in
// the tile by (record, entry index): the samples of the channel in the lanes below -- per entry, the ballot's bits below the lane,
// added up in the lane's own column of an LDS matrix, whoever fires --, then those of the lane's own earlier entries: the column's
// cell counts on as the lane places its samples in ascending entry order.  No place comes from an atomic.  Every sample's value goes to
// vals[place] (`limit` of them exist), the first cap samples to out.
__global__ void __launch_bounds__(TIP_SUBCOM_TILE) k_subcom_place(SubcomSrc S, SubcomRule R, unsigned long long n, unsigned long long tiles,
                                                                  const unsigned *__restrict__ marks, const unsigned *__restrict__ base,
                                                                  const unsigned long long *__restrict__ offsets, TipSubcomSample *__restrict__ out,
                                                                  unsigned long long cap, uint8_t *__restrict__ vals, unsigned long long limit)
{
    __shared__ TipSubcomEntry s_tab[TIP_SUBCOM_MAX_ENTRIES];
    __shared__ uint16_t s_below[TIP_SUBCOM_MAX_CHANNELS * TIP_SUBCOM_TILE];      // (at most 63 lanes x 256 entries + 256 of its own)
    __shared__ unsigned long long s_at[TIP_SUBCOM_MAX_CHANNELS];
    const unsigned long long tile = blockIdx.x, i = tile * TIP_SUBCOM_TILE + threadIdx.x;
    const int lane = (int)threadIdx.x;
    subcom_load_table(s_tab, R);
    for (int c = lane; c < R.nchan; c += TIP_SUBCOM_TILE) s_at[c] = offsets[c] + base[(unsigned long long)c * tiles + tile];
    for (int k = lane; k < R.nchan * TIP_SUBCOM_TILE; k += TIP_SUBCOM_TILE) s_below[k] = 0;
    __syncthreads();
    const unsigned m = i < n ? marks[i] : 0u;
    if (!__ballot(m & TIP_SUBCOM_M_USED)) return;
    const unsigned long long below = (1ull << lane) - 1;
    for (int e = 0; e < R.ne; e++) {
        const TipSubcomEntry E = s_tab[e];
        unsigned fl;
        bool drop;
        const unsigned long long bx = __ballot(subcom_exists(E, m, R.trusted_only, &fl, &drop));
        if (bx) s_below[E.channel * TIP_SUBCOM_TILE + lane] += (uint16_t)__popcll(bx & below);
    }
    if (!(m & TIP_SUBCOM_M_USED)) return;                    // (a lane's column is its own: no barrier between the passes)
    const unsigned char *r = S.recs + i * S.stride + S.o_bytes;
    const double t = *reinterpret_cast<const double *>(S.times + i * S.tstride);
    for (int e = 0; e < R.ne; e++) {
        const TipSubcomEntry E = s_tab[e];
        unsigned fl;
        bool drop;
        if (!subcom_exists(E, m, R.trusted_only, &fl, &drop)) continue;
        const unsigned long long at = s_at[E.channel] + s_below[E.channel * TIP_SUBCOM_TILE + lane]++;
        const TipSubcomSample s = tip_subcom_sample(t, (uint32_t)i, tip_subcom_mark_id(m), E, e, r[E.byte], fl);
        if (at < limit) vals[at] = s.value;
        if (at < cap) out[at] = s;
    }
}

// Stage 5, a lane per placed sample: its channel by a search of offsets (in LDS), its two neighbours within the channel's range, bit 8.
// The spike count goes by atomic add.
__global__ void __launch_bounds__(256) k_subcom_spikes(int nchan, int thr, const unsigned long long *__restrict__ offsets, const uint8_t *__restrict__ vals,
                                                       unsigned long long limit, TipSubcomSample *__restrict__ out, unsigned long long cap,
                                                       unsigned long long *__restrict__ sum)
{
    __shared__ unsigned long long s_off[TIP_SUBCOM_MAX_CHANNELS + 1];
    for (int c = (int)threadIdx.x; c <= nchan; c += 256) s_off[c] = offsets[c];
    __syncthreads();
    const unsigned long long p = (unsigned long long)blockIdx.x * 256 + threadIdx.x, total = s_off[nchan] < limit ? s_off[nchan] : limit;
    bool spike = false;
    if (p < total) {
        int lo = 0, hi = nchan;                                  // the first k with s_off[k] > p lies in (lo, hi]
        while (hi - lo > 1) {
            const int mid = (lo + hi) >> 1;
            if (s_off[mid] > p) hi = mid;
            else lo = mid;
        }
        spike = p > s_off[lo] && p + 1 < s_off[hi] && tip_subcom_is_spike(vals[p - 1], vals[p], vals[p + 1], thr);
        if (spike && p < cap) out[p].flags |= (uint8_t)TIP_SUBCOM_SPIKE;
    }
    const unsigned c = (unsigned)__popcll(__ballot(spike));
    if ((threadIdx.x & 63) == 0 && c) atomicAdd(&sum[SUBCOM_C_SPIKES], (unsigned long long)c);
}

}  // namespace pdt

using namespace pdt;

namespace pdtrt {

extern const char *const tip_subcom_kernel_names[5] = { "k_subcom_mark", "k_subcom_count", "k_subcom_scan", "k_subcom_place", "k_subcom_spikes" };

// The five kernels over n records that are on the device (n >= 1).  chain_layout: the records are the chain's own (TipDcsChainRec) and
// their time stamps lie at times_dev, one double each; otherwise they are pdt_frame records.  sum: 128 zeroed bytes; table_dev: the ne
// entries; marks: n words; cnt: nchan * tiles words, tiles = ceil(n / 64); offsets: nchan + 1 words of 64 bits; vals: `limit` bytes,
// limit >= the samples there can be; out: cap samples.
hipError_t tip_subcom_launch(hipStream_t st, const void *recs_dev, bool chain_layout, const void *times_dev, unsigned long long n, const void *table_dev, int ne,
                             int nchan, int trusted_only, int thr, void *sum_dev, void *marks_dev, void *cnt_dev, void *offsets_dev, void *vals_dev,
                             unsigned long long limit, void *out_dev, unsigned long long cap, hipEvent_t *inner)
{
    SubcomSrc S;
    S.recs = (const unsigned char *)recs_dev;
    if (chain_layout) {
        S.times = (const unsigned char *)times_dev;
        S.stride = sizeof(TipDcsChainRec), S.tstride = sizeof(double), S.o_nbytes = offsetof(TipDcsChainRec, nbytes), S.o_bytes = offsetof(TipDcsChainRec, bytes);
    } else {
        S.times = S.recs + offsetof(TipDcsRec, time);
        S.stride = S.tstride = sizeof(TipDcsRec), S.o_nbytes = offsetof(TipDcsRec, nbytes), S.o_bytes = offsetof(TipDcsRec, bytes);
    }
    const SubcomRule R{ (const TipSubcomEntry *)table_dev, ne, nchan, trusted_only, thr };
    const unsigned long long tiles = (n + TIP_SUBCOM_TILE - 1) / TIP_SUBCOM_TILE;
    hipLaunchKernelGGL(k_subcom_mark, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, S, n, (unsigned *)marks_dev);
    if (inner) (void)hipEventRecord(inner[0], st);
    hipLaunchKernelGGL(k_subcom_count, dim3((unsigned)tiles), dim3(TIP_SUBCOM_TILE), 0, st, R, n, tiles, (const unsigned *)marks_dev, (unsigned *)cnt_dev,
                       (unsigned long long *)sum_dev);
    if (inner) (void)hipEventRecord(inner[1], st);
    hipLaunchKernelGGL(k_subcom_scan, dim3(1), dim3(SUBCOM_SCAN_THREADS), 0, st, nchan, tiles, (unsigned *)cnt_dev, (unsigned long long *)offsets_dev,
                       (unsigned long long *)sum_dev);
    if (inner) (void)hipEventRecord(inner[2], st);
    hipLaunchKernelGGL(k_subcom_place, dim3((unsigned)tiles), dim3(TIP_SUBCOM_TILE), 0, st, S, R, n, tiles, (const unsigned *)marks_dev, (const unsigned *)cnt_dev,
                       (const unsigned long long *)offsets_dev, (TipSubcomSample *)out_dev, cap, (uint8_t *)vals_dev, limit);
    if (inner) (void)hipEventRecord(inner[3], st);
    hipLaunchKernelGGL(k_subcom_spikes, dim3((unsigned)((limit + 255) / 256)), dim3(256), 0, st, nchan, thr, (const unsigned long long *)offsets_dev,
                       (const uint8_t *)vals_dev, limit, (TipSubcomSample *)out_dev, cap, (unsigned long long *)sum_dev);
    return hipGetLastError();
}

// the counters the kernels left -> the summary
void tip_subcom_summary(const unsigned long long *c, pdt_subcom_summary *s)
{
    s->used = c[SUBCOM_C_USED];
    s->skipped = c[SUBCOM_C_SKIPPED];
    s->bad_id = c[SUBCOM_C_BAD_ID];
    s->samples = c[SUBCOM_C_SAMPLES];
    s->dropped = c[SUBCOM_C_DROPPED];
    s->byte_parity = c[SUBCOM_C_BYTE_PARITY];
    s->id_parity = c[SUBCOM_C_ID_PARITY];
    s->spikes = c[SUBCOM_C_SPIKES];
    s->channels_hit = c[SUBCOM_C_HIT];
}

// table and cfg -> nchan, the most entries that fire in a record, thr; PDT_ERR_ARG for what is not allowed, or for more than 2^31 - 1
// samples that n records could give
int tip_subcom_rule(const pdt_subcom_entry *entries, uint64_t nentries, const pdt_subcom_cfg *cfg, uint64_t n, int *nchan, int *max_fire, int *trusted_only, int *thr)
{
    *nchan = tip_subcom_table_channels(reinterpret_cast<const TipSubcomEntry *>(entries), nentries);
    *thr = tip_subcom_threshold(cfg ? cfg->spike_threshold : 0u);
    *trusted_only = cfg && cfg->trusted_only;
    if (!*nchan || *thr < 0) return PDT_ERR_ARG;
    *max_fire = tip_subcom_table_max_fire(reinterpret_cast<const TipSubcomEntry *>(entries), (int)nentries);
    return n * (uint64_t)*max_fire >= (1ull << 31) ? PDT_ERR_ARG : PDT_OK;
}

}  // namespace pdtrt

extern "C" {

int pdt_tip_subcom_tile(void) { return TIP_SUBCOM_TILE; }

int pdt_subcom_table(int which, pdt_subcom_entry *entries, int cap)
{
    TipSubcomEntry t[TIP_SUBCOM_MAX_ENTRIES];
    const int n = tip_subcom_builtin(which, t);
    if (entries && cap > 0) memcpy(entries, t, (size_t)std::min(n, cap) * sizeof *t);
    return n;
}

const char *pdt_subcom_name(int which, int channel) { return tip_subcom_builtin_name(which, channel); }

int pdt_host_tip_subcom(const pdt_frame *frames, uint64_t n, const pdt_subcom_entry *entries, uint64_t nentries, const pdt_subcom_cfg *cfg, pdt_subcom_sample *out,
                        int cap, int *count, uint64_t *offsets, pdt_subcom_summary *summary)
{
    int nchan, max_fire, trusted, thr;
    if (!count || !summary || (!frames && n) || n >= (1ull << 31) || cap < 0 || (!out && cap)) return PDT_ERR_ARG;
    if (pdtrt::tip_subcom_rule(entries, nentries, cfg, n, &nchan, &max_fire, &trusted, &thr)) return PDT_ERR_ARG;
    try {
        const TipDcsRec *recs = reinterpret_cast<const TipDcsRec *>(frames);
        const TipSubcomEntry *tab = reinterpret_cast<const TipSubcomEntry *>(entries);
        TipSubcomSummary *sum = reinterpret_cast<TipSubcomSummary *>(summary);
        std::vector<uint64_t> off((size_t)nchan + 1), cursor((size_t)nchan);
        tip_subcom_host_count(recs, n, tab, (int)nentries, nchan, trusted != 0, off.data(), sum);
        std::vector<uint8_t> V((size_t)off[(size_t)nchan] + 1);
        tip_subcom_host_fill(recs, n, tab, (int)nentries, nchan, trusted != 0, thr, off.data(), cursor.data(), V.data(), reinterpret_cast<TipSubcomSample *>(out),
                             (uint64_t)cap, sum);
        if (offsets) memcpy(offsets, off.data(), off.size() * sizeof(uint64_t));
        *count = (int)sum->samples;
    } catch (const std::exception &) { return PDT_ERR_NOMEM; }
    return PDT_OK;
}

// one line per sample: "%.5f %s %u %u %s\n" -- the time, the channel's name in table `which` (c<channel> where it has none: a caller's
// table), the counter, the value, the flags as a subset of the letters b i u s in that order, or "-"
static void subcom_text(const pdt_subcom_sample *p, uint64_t n, int which, std::string &s)
{
    char b[96];
    for (uint64_t i = 0; i < n; i++) {
        const pdt_subcom_sample &m = p[i];
        char name[16], fl[8];
        const char *known = tip_subcom_builtin_name(which, m.channel);
        if (known) snprintf(name, sizeof name, "%s", known);
        else snprintf(name, sizeof name, "c%u", (unsigned)m.channel);
        int k = 0;
        if (m.flags & PDT_SUBCOM_BYTE_PARITY) fl[k++] = 'b';
        if (m.flags & PDT_SUBCOM_ID_PARITY) fl[k++] = 'i';
        if (m.flags & PDT_SUBCOM_UNCOVERED) fl[k++] = 'u';
        if (m.flags & PDT_SUBCOM_SPIKE) fl[k++] = 's';
        if (!k) fl[k++] = '-';
        fl[k] = 0;
        snprintf(b, sizeof b, "%.5f %s %u %u %s\n", m.time, name, (unsigned)m.minor_id, (unsigned)m.value, fl);
        s += b;
    }
}

uint64_t pdt_format_subcom(const pdt_subcom_sample *samples, uint64_t n, int which, char *buf, uint64_t cap)
{
    if (!samples && n) return 0;
    try {
        std::string s;
        subcom_text(samples, n, which, s);
        if (buf && cap) memcpy(buf, s.data(), (size_t)std::min<uint64_t>(cap, s.size()));
        return s.size();
    } catch (const std::exception &) { return 0; }
}

int pdt_write_subcom(const pdt_subcom_sample *samples, uint64_t n, int which, int fd, uint64_t *bytes_written)
{
    if (bytes_written) *bytes_written = 0;
    if ((!samples && n) || fd < 0) return PDT_ERR_ARG;
    try {
        std::string s;
        subcom_text(samples, n, which, s);
        size_t at = 0;
        while (at < s.size()) {
            const ssize_t r = write(fd, s.data() + at, s.size() - at);
            if (r < 0 && errno == EINTR) continue;
            if (r <= 0) return PDT_ERR_IO;
            at += (size_t)r;
        }
        if (bytes_written) *bytes_written = s.size();
        return PDT_OK;
    } catch (const std::exception &) { return PDT_ERR_NOMEM; }
}

}  // extern "C"
