// pdt_tip_dcs.hip -- decommutation of TIP minor frames into the DCS-2 platform messages (pdt_tip_dcs.h): the kernels k_dcs_gather,
// k_dcs_maps, k_dcs_scan and k_dcs_pack, their launch, the host restatement pdt_host_tip_dcs and the packets' text.  A unit of its
// own, beside pdt_tip_repair.hip.
#include <hip/hip_runtime.h>
#include <errno.h>
#include <unistd.h>
#include <algorithm>
#include <exception>
#include <string>
#include <vector>

#include "../../include/pdt.h"
#include "pdt_tip_dcs.h"

static_assert(sizeof(pdt_frame) == sizeof(pdt::TipDcsRec) && sizeof(pdt_frame) == 136, "pdt_frame");
static_assert(offsetof(pdt_frame, bit_index) == offsetof(pdt::TipDcsRec, bit_index) && offsetof(pdt_frame, nbytes) == offsetof(pdt::TipDcsRec, nbytes) &&
              offsetof(pdt_frame, complete) == offsetof(pdt::TipDcsRec, complete) && offsetof(pdt_frame, bytes) == offsetof(pdt::TipDcsRec, bytes), "pdt_frame");
static_assert(sizeof(pdt_dcs_packet) == sizeof(pdt::TipDcsPacket) && sizeof(pdt_dcs_packet) == 88, "pdt_dcs_packet");
static_assert(offsetof(pdt_dcs_packet, stream_index) == offsetof(pdt::TipDcsPacket, stream_index) && offsetof(pdt_dcs_packet, frame) == offsetof(pdt::TipDcsPacket, frame) &&
              offsetof(pdt_dcs_packet, time_code) == offsetof(pdt::TipDcsPacket, time_code) && offsetof(pdt_dcs_packet, id) == offsetof(pdt::TipDcsPacket, id) &&
              offsetof(pdt_dcs_packet, doppler_raw) == offsetof(pdt::TipDcsPacket, doppler_raw) && offsetof(pdt_dcs_packet, slot) == offsetof(pdt::TipDcsPacket, slot) &&
              offsetof(pdt_dcs_packet, doppler_ok) == offsetof(pdt::TipDcsPacket, doppler_ok) && offsetof(pdt_dcs_packet, bytes) == offsetof(pdt::TipDcsPacket, bytes) &&
              offsetof(pdt_dcs_packet, bytes) == 40, "pdt_dcs_packet");
static_assert(sizeof(pdt_dcs_summary) == sizeof(pdt::TipDcsSummary) && sizeof(pdt_dcs_summary) == 80, "pdt_dcs_summary");
static_assert(sizeof(pdt_dcs_cfg) == 8, "pdt_dcs_cfg");

namespace pdt {

// Where the records are: the caller's pdt_frame records, or the chain's own (bit index first, no time stamp: the stamps come up from the
// host beside them).  Strides and offsets in bytes; the flags are nbytes and, behind it, complete.
struct DcsSrc {
    const unsigned char *recs, *times;
    unsigned stride, tstride, o_bit, o_nbytes, o_bytes;
};

// the counters on the device (DcsWork's first region)
enum { DCS_C_USED = 0, DCS_C_SEGMENTS, DCS_C_HEADS, DCS_C_BAD, DCS_C_PACKETS, DCS_C_COMPLETE, DCS_C_DOPPLER_BAD, DCS_C_COUNT };

// a tile as a map: entered with s = 0 .. 43 bytes still owned by the open packet, it is left with exit[s] and accepts cnt[s] heads
constexpr int DCS_STATES = TIP_DCS_MAXLEN;
struct DcsTileMap {
    unsigned elig;                 // eligible records of the tile
    uint16_t cnt[DCS_STATES];
    uint8_t exit[DCS_STATES];
};
// ... and what the scan leaves for it: the packets and the eligible records in front of it, its true entry state
struct DcsTileEntry {
    unsigned long long packets, elig;
    unsigned state, pad;
};
enum { DCS_F_ELIGIBLE = 1, DCS_F_START = 2 };

__device__ __forceinline__ bool dcs_eligible(const DcsSrc &S, unsigned long long i)
{
    const unsigned char *f = S.recs + i * S.stride + S.o_nbytes;
    return tip_dcs_eligible(f[1], f[0]);
}
__device__ __forceinline__ long long dcs_bit(const DcsSrc &S, unsigned long long i) { return *reinterpret_cast<const long long *>(S.recs + i * S.stride + S.o_bit); }
__device__ __forceinline__ unsigned dcs_byte(const DcsSrc &S, unsigned long long i, int slot) { return S.recs[i * S.stride + S.o_bytes + tip_dcs_slot_byte(slot)]; }
// record j continues record j - 1
__device__ __forceinline__ bool dcs_continues(const DcsSrc &S, unsigned long long j, unsigned long long n)
{
    return j > 0 && j < n && dcs_eligible(S, j) && dcs_eligible(S, j - 1) && dcs_bit(S, j) - dcs_bit(S, j - 1) == TIP_DCS_FRAME_BITS;
}

// Stage 1, a lane per stream byte (32 per record, ineligible records as 32 zeros that belong to no segment; the grid covers whole
// tiles): the byte goes to the stream, a record's first lane writes its flags, and every byte is tested for "head" and for "bad code"
// -- the two bytes behind it come from the next record where that one continues this one.  Both answers leave as ballots.
__global__ void __launch_bounds__(256) k_dcs_gather(DcsSrc S, unsigned long long n, unsigned channel_max, uint8_t *__restrict__ stream,
                                                    uint8_t *__restrict__ flags, unsigned long long *__restrict__ head, unsigned long long *__restrict__ bad)
{
    const unsigned long long p = (unsigned long long)blockIdx.x * 256 + threadIdx.x, i = p >> 5;
    const int slot = (int)(p & 31);
    const bool el = i < n && dcs_eligible(S, i);
    const unsigned b0 = el ? dcs_byte(S, i, slot) : 0u;
    int what = 0;
    if (b0 == 0xD6u) {
        const bool inside = slot + 2 < TIP_DCS_SLOTS;
        if (inside || dcs_continues(S, i + 1, n)) {
            const unsigned b1 = slot + 1 < TIP_DCS_SLOTS ? dcs_byte(S, i, slot + 1) : dcs_byte(S, i + 1, 0);
            const unsigned b2 = inside ? dcs_byte(S, i, slot + 2) : dcs_byte(S, i + 1, slot + 2 - TIP_DCS_SLOTS);
            what = tip_dcs_classify(b0, b1, b2, channel_max);
        }
    }
    stream[p] = (uint8_t)b0;
    if (slot == 0 && i < n) flags[i] = el ? (uint8_t)(DCS_F_ELIGIBLE | (dcs_continues(S, i, n) ? 0 : DCS_F_START)) : (uint8_t)0;
    const unsigned long long h = __ballot(what == 1), b = __ballot(what == 2);
    if ((threadIdx.x & 63) == 0) {
        head[p >> 6] = h;
        bad[p >> 6] = b;
    }
}

// What stages 2 and 4 share, one wavefront per tile, lane = record of the tile = 32-bit word of its bitmaps.  The tile's head words and
// its records' flags (two more behind it) go to LDS; every head gets the bytes its packet owns: L, cut at the segment's end.
struct DcsTileLds {
    unsigned head[TIP_DCS_TILE_RECS];
    unsigned acc[TIP_DCS_TILE_RECS];
    uint8_t flags[TIP_DCS_TILE_RECS + 2];
    uint8_t own[TIP_DCS_TILE];
};
__device__ __forceinline__ bool dcs_flag_continues(unsigned f) { return (f & DCS_F_ELIGIBLE) && !(f & DCS_F_START); }
__device__ __forceinline__ void dcs_tile_load(DcsTileLds &T, unsigned long long tile, unsigned long long n, const uint8_t *__restrict__ stream,
                                              const uint8_t *__restrict__ flags, const unsigned *__restrict__ head)
{
    const int lane = (int)threadIdx.x;
    const unsigned long long r0 = tile * TIP_DCS_TILE_RECS;
    const unsigned w = head[r0 + lane];
    T.head[lane] = w;
    T.acc[lane] = 0;
    T.flags[lane] = r0 + lane < n ? flags[r0 + lane] : (uint8_t)0;
    if (lane < 2) T.flags[TIP_DCS_TILE_RECS + lane] = r0 + TIP_DCS_TILE_RECS + lane < n ? flags[r0 + TIP_DCS_TILE_RECS + lane] : (uint8_t)0;
    __syncthreads();
    int left = 0;                                            // bytes of the segment behind this record (64 is as good as any more)
    if (dcs_flag_continues(T.flags[lane + 1])) left = dcs_flag_continues(T.flags[lane + 2]) ? 2 * TIP_DCS_SLOTS : TIP_DCS_SLOTS;
    for (unsigned m = w; m; m &= m - 1) {
        const int bit = __builtin_ctz(m), k = lane * TIP_DCS_SLOTS + bit;
        const int L = tip_dcs_len((unsigned)stream[tile * TIP_DCS_TILE + k + 2] >> 4), room = TIP_DCS_SLOTS - bit + left;   // (a head: k + 2 is inside)
        T.own[k] = (uint8_t)(L < room ? L : room);
    }
    __syncthreads();
}

// The heads accepted from position `cur` of the tile on: each accepted head moves `cur` behind its packet, the next one is the first
// head at or behind `cur`.  mark: set the accepted heads' bits in T.acc.  Returns the bytes the last packet owns of the next tile.
__device__ __forceinline__ int dcs_tile_walk(DcsTileLds &T, int cur, bool mark, unsigned *count)
{
    unsigned c = 0;
    int w = cur >> 5;
    unsigned m = T.head[w] & (~0u << (cur & 31));
    for (;;) {
        while (!m && ++w < TIP_DCS_TILE_RECS) m = T.head[w];
        if (!m) break;
        const int bit = __builtin_ctz(m), k = w * TIP_DCS_SLOTS + bit;
        if (mark) T.acc[w] |= 1u << bit;
        c++;
        cur = k + T.own[k];
        w = cur >> 5;
        if (w >= TIP_DCS_TILE_RECS) break;
        m = T.head[w] & (~0u << (cur & 31));
    }
    *count = c;
    return cur > TIP_DCS_TILE ? cur - TIP_DCS_TILE : 0;
}

__device__ __forceinline__ unsigned dcs_wave_sum(unsigned v)
{
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) v += __shfl_xor(v, d);
    return v;
}

// Stage 2: the tile's map.  Lane s = 0 .. 43 walks the tile as if s bytes of it were owned on entry.  The tile's counts go by atomics.
__global__ void __launch_bounds__(64) k_dcs_maps(unsigned long long n, const uint8_t *__restrict__ stream, const uint8_t *__restrict__ flags,
                                                 const unsigned *__restrict__ head, const unsigned *__restrict__ bad, DcsTileMap *__restrict__ maps,
                                                 unsigned long long *__restrict__ sum)
{
    __shared__ DcsTileLds T;
    const unsigned long long tile = blockIdx.x;
    const int lane = (int)threadIdx.x;
    dcs_tile_load(T, tile, n, stream, flags, head);
    const unsigned f = T.flags[lane];
    const unsigned used = (unsigned)__popcll(__ballot(f & DCS_F_ELIGIBLE)), starts = (unsigned)__popcll(__ballot(f & DCS_F_START));
    const unsigned heads = dcs_wave_sum((unsigned)__popc(T.head[lane])), bads = dcs_wave_sum((unsigned)__popc(bad[tile * TIP_DCS_TILE_RECS + lane]));
    if (lane < DCS_STATES) {
        unsigned c;
        const int e = dcs_tile_walk(T, lane, false, &c);
        maps[tile].exit[lane] = (uint8_t)e;
        maps[tile].cnt[lane] = (uint16_t)c;
    }
    if (lane == 0) {
        maps[tile].elig = used;
        if (used) atomicAdd(&sum[DCS_C_USED], (unsigned long long)used);
        if (starts) atomicAdd(&sum[DCS_C_SEGMENTS], (unsigned long long)starts);
        if (heads) atomicAdd(&sum[DCS_C_HEADS], (unsigned long long)heads);
        if (bads) atomicAdd(&sum[DCS_C_BAD], (unsigned long long)bads);
    }
}

// Stage 3, one workgroup: the maps composed in order.  Thread t composes the maps of its stretch of tiles (a map of 44 entries in LDS),
// thread 0 carries the one true state through the 256 stretches, then every thread carries it through its own tiles and leaves each
// tile its entry: state, packets and eligible records in front of it.  The packet count stays here, in the counters.
constexpr int DCS_SCAN_THREADS = 256;
__global__ void __launch_bounds__(DCS_SCAN_THREADS) k_dcs_scan(unsigned long long ntiles, const DcsTileMap *__restrict__ maps, DcsTileEntry *__restrict__ entry,
                                                               unsigned long long *__restrict__ sum)
{
    __shared__ unsigned s_cnt[DCS_SCAN_THREADS][DCS_STATES];
    __shared__ uint8_t s_exit[DCS_SCAN_THREADS][DCS_STATES];
    __shared__ unsigned long long s_elig[DCS_SCAN_THREADS], s_in_packets[DCS_SCAN_THREADS], s_in_elig[DCS_SCAN_THREADS];
    __shared__ unsigned s_in_state[DCS_SCAN_THREADS];
    const unsigned t = threadIdx.x;
    const unsigned long long each = (ntiles + DCS_SCAN_THREADS - 1) / DCS_SCAN_THREADS;
    const unsigned long long lo = t * each < ntiles ? t * each : ntiles, hi = lo + each < ntiles ? lo + each : ntiles;
    for (int s = 0; s < DCS_STATES; s++) {
        s_cnt[t][s] = 0;
        s_exit[t][s] = (uint8_t)s;
    }
    unsigned long long el = 0;
    for (unsigned long long k = lo; k < hi; k++) {
        const DcsTileMap &M = maps[k];
        for (int s = 0; s < DCS_STATES; s++) {
            const unsigned e = s_exit[t][s];
            s_cnt[t][s] += M.cnt[e];
            s_exit[t][s] = M.exit[e];
        }
        el += M.elig;
    }
    s_elig[t] = el;
    __syncthreads();
    if (t == 0) {
        unsigned state = 0;
        unsigned long long packets = 0, elig = 0;
        for (int c = 0; c < DCS_SCAN_THREADS; c++) {
            s_in_state[c] = state;
            s_in_packets[c] = packets;
            s_in_elig[c] = elig;
            packets += s_cnt[c][state];
            state = s_exit[c][state];
            elig += s_elig[c];
        }
        sum[DCS_C_PACKETS] = packets;
    }
    __syncthreads();
    unsigned state = s_in_state[t];
    unsigned long long packets = s_in_packets[t], elig = s_in_elig[t];
    for (unsigned long long k = lo; k < hi; k++) {
        const DcsTileMap &M = maps[k];
        entry[k] = DcsTileEntry{ packets, elig, state, 0u };
        packets += M.cnt[state];
        state = M.exit[state];
        elig += M.elig;
    }
}

// Stage 4: a tile marks its accepted heads from its true entry state; the marks' counts, scanned across the wavefront, are the
// packets' places behind the tile's first; every lane packs the packets of its record.  At most cap packets are written.
__global__ void __launch_bounds__(64) k_dcs_pack(DcsSrc S, unsigned long long n, const uint8_t *__restrict__ stream, const uint8_t *__restrict__ flags,
                                                 const unsigned *__restrict__ head, const DcsTileEntry *__restrict__ entry, TipDcsPacket *__restrict__ out,
                                                 unsigned long long cap, unsigned long long *__restrict__ sum)
{
    __shared__ DcsTileLds T;
    const unsigned long long tile = blockIdx.x;
    const int lane = (int)threadIdx.x;
    dcs_tile_load(T, tile, n, stream, flags, head);
    const DcsTileEntry E = entry[tile];
    if (lane == 0) {
        unsigned c;
        (void)dcs_tile_walk(T, (int)E.state, true, &c);
    }
    __syncthreads();
    const unsigned a = T.acc[lane];
    unsigned before = (unsigned)__popc(a);
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const unsigned o = __shfl_up(before, d);
        if (lane >= d) before += o;
    }
    before -= (unsigned)__popc(a);
    const unsigned long long el = __ballot(T.flags[lane] & DCS_F_ELIGIBLE);
    const unsigned long long rec = tile * TIP_DCS_TILE_RECS + lane;
    const long long first = (long long)(E.elig + (unsigned long long)__popcll(el & ((1ull << lane) - 1))) * TIP_DCS_SLOTS;
    unsigned complete = 0, odd = 0;
    unsigned long long at = E.packets + before;
    for (unsigned m = a; m; m &= m - 1, at++) {
        const int bit = __builtin_ctz(m), k = lane * TIP_DCS_SLOTS + bit, own = T.own[k];
        const uint8_t *s = stream + tile * TIP_DCS_TILE + k;
        const int L = tip_dcs_len((unsigned)s[2] >> 4);
        if (own == L) {
            complete++;
            odd += !tip_dcs_even(tip_dcs_doppler_word(s, L));
        }
        if (at < cap) tip_dcs_packet(out + at, s, own, *reinterpret_cast<const double *>(S.times + rec * S.tstride), (uint32_t)rec, bit, first + bit);
    }
    complete = dcs_wave_sum(complete);
    odd = dcs_wave_sum(odd);
    if (lane == 0) {
        if (complete) atomicAdd(&sum[DCS_C_COMPLETE], (unsigned long long)complete);
        if (odd) atomicAdd(&sum[DCS_C_DOPPLER_BAD], (unsigned long long)odd);
    }
}

}  // namespace pdt

using namespace pdt;

namespace pdtrt {

extern const char *const tip_dcs_kernel_names[4] = { "k_dcs_gather", "k_dcs_maps", "k_dcs_scan", "k_dcs_pack" };

size_t tip_dcs_map_bytes() { return sizeof(DcsTileMap); }
size_t tip_dcs_entry_bytes() { return sizeof(DcsTileEntry); }

// The four kernels over n records that are on the device (n >= 1).  chain_layout: the records are the chain's own (TipDcsChainRec) and
// their time stamps lie at times_dev, one double each; otherwise they are pdt_frame records.
// sum: 128 zeroed bytes; flags: n + 2 zeroed bytes; the other regions as DcsWork lays them out for `tiles` = ceil(n / 64) tiles.
hipError_t tip_dcs_launch(hipStream_t st, const void *recs_dev, bool chain_layout, const void *times_dev, unsigned long long n, unsigned channel_max,
                          void *sum_dev, void *flags_dev, void *stream_dev, void *head_dev, void *bad_dev, void *maps_dev, void *entry_dev, void *out_dev,
                          unsigned long long cap, hipEvent_t *inner)
{
    DcsSrc S;
    S.recs = (const unsigned char *)recs_dev;
    if (chain_layout) {
        S.times = (const unsigned char *)times_dev;
        S.stride = sizeof(TipDcsChainRec), S.tstride = sizeof(double), S.o_bit = offsetof(TipDcsChainRec, bit_index), S.o_nbytes = offsetof(TipDcsChainRec, nbytes),
        S.o_bytes = offsetof(TipDcsChainRec, bytes);
    } else {
        S.times = S.recs + offsetof(TipDcsRec, time);
        S.stride = S.tstride = sizeof(TipDcsRec), S.o_bit = offsetof(TipDcsRec, bit_index), S.o_nbytes = offsetof(TipDcsRec, nbytes), S.o_bytes = offsetof(TipDcsRec, bytes);
    }
    const unsigned long long tiles = (n + TIP_DCS_TILE_RECS - 1) / TIP_DCS_TILE_RECS;
    hipLaunchKernelGGL(k_dcs_gather, dim3((unsigned)(tiles * (TIP_DCS_TILE / 256))), dim3(256), 0, st, S, n, channel_max, (uint8_t *)stream_dev, (uint8_t *)flags_dev,
                       (unsigned long long *)head_dev, (unsigned long long *)bad_dev);
    if (inner) (void)hipEventRecord(inner[0], st);
    hipLaunchKernelGGL(k_dcs_maps, dim3((unsigned)tiles), dim3(64), 0, st, n, (const uint8_t *)stream_dev, (const uint8_t *)flags_dev, (const unsigned *)head_dev,
                       (const unsigned *)bad_dev, (DcsTileMap *)maps_dev, (unsigned long long *)sum_dev);
    if (inner) (void)hipEventRecord(inner[1], st);
    hipLaunchKernelGGL(k_dcs_scan, dim3(1), dim3(DCS_SCAN_THREADS), 0, st, tiles, (const DcsTileMap *)maps_dev, (DcsTileEntry *)entry_dev, (unsigned long long *)sum_dev);
    if (inner) (void)hipEventRecord(inner[2], st);
    hipLaunchKernelGGL(k_dcs_pack, dim3((unsigned)tiles), dim3(64), 0, st, S, n, (const uint8_t *)stream_dev, (const uint8_t *)flags_dev, (const unsigned *)head_dev,
                       (const DcsTileEntry *)entry_dev, (TipDcsPacket *)out_dev, cap, (unsigned long long *)sum_dev);
    return hipGetLastError();
}

// the counters the kernels left -> the summary (n records went in)
void tip_dcs_summary(const unsigned long long *c, unsigned long long n, pdt_dcs_summary *s)
{
    s->used = c[DCS_C_USED];
    s->skipped = n - c[DCS_C_USED];
    s->segments = c[DCS_C_SEGMENTS];
    s->stream_bytes = c[DCS_C_USED] * TIP_DCS_SLOTS;
    s->heads = c[DCS_C_HEADS];
    s->bad_code = c[DCS_C_BAD];
    s->packets = c[DCS_C_PACKETS];
    s->shadowed = c[DCS_C_HEADS] - c[DCS_C_PACKETS];
    s->complete = c[DCS_C_COMPLETE];
    s->doppler_bad = c[DCS_C_DOPPLER_BAD];
}

// cfg -> the channel byte's bound; PDT_ERR_ARG for a value that is not allowed
int tip_dcs_rule(const pdt_dcs_cfg *cfg, unsigned *channel_max)
{
    *channel_max = tip_dcs_channel_max(cfg ? cfg->channel_max : 0u);
    return *channel_max ? PDT_OK : PDT_ERR_ARG;
}

}  // namespace pdtrt

extern "C" {

int pdt_tip_dcs_tile(void) { return TIP_DCS_TILE; }

int pdt_host_tip_dcs(const pdt_frame *frames, uint64_t n, const pdt_dcs_cfg *cfg, pdt_dcs_packet *out, int cap, int *count, pdt_dcs_summary *summary)
{
    unsigned channel_max;
    if (!count || !summary || (!frames && n) || n >= (1ull << 31) || cap < 0 || (!out && cap) || pdtrt::tip_dcs_rule(cfg, &channel_max)) return PDT_ERR_ARG;
    try {
        std::vector<uint8_t> S((size_t)n * TIP_DCS_SLOTS + 1);
        const uint64_t found = tip_dcs_host(reinterpret_cast<const TipDcsRec *>(frames), n, channel_max, S.data(), reinterpret_cast<TipDcsPacket *>(out), (uint64_t)cap,
                                            reinterpret_cast<TipDcsSummary *>(summary));
        *count = (int)std::min<uint64_t>(found, 0x7fffffffull);
    } catch (const std::exception &) { return PDT_ERR_NOMEM; }
    return PDT_OK;
}

// one line per packet: "%.5f %u %u %07u %08X %s " (time, channel, blocks, time_code, id, Doppler), "%02X " per byte, "\n".  The Doppler is
// "%.5f" of doppler_raw / 32.0 -- behind a '*' when the word's parity is odd --, or "-" for a packet that is cut off
static void dcs_text(const pdt_dcs_packet *p, uint64_t n, std::string &s)
{
    char b[96];
    for (uint64_t i = 0; i < n; i++) {
        const pdt_dcs_packet &m = p[i];
        char d[40];
        if (!m.complete) snprintf(d, sizeof d, "-");
        else snprintf(d, sizeof d, "%s%.5f", m.doppler_ok ? "" : "*", (double)m.doppler_raw / 32.0);
        snprintf(b, sizeof b, "%.5f %u %u %07u %08X %s ", m.time, (unsigned)m.channel, (unsigned)m.blocks, (unsigned)m.time_code, (unsigned)m.id, d);
        s += b;
        const int nb = m.nbytes < TIP_DCS_MAXLEN ? m.nbytes : TIP_DCS_MAXLEN;
        for (int k = 0; k < nb; k++) {
            snprintf(b, sizeof b, "%02X ", (unsigned)m.bytes[k]);
            s += b;
        }
        s += '\n';
    }
}

uint64_t pdt_format_dcs_packets(const pdt_dcs_packet *packets, uint64_t n, char *buf, uint64_t cap)
{
    if (!packets && n) return 0;
    try {
        std::string s;
        dcs_text(packets, n, s);
        if (buf && cap) memcpy(buf, s.data(), (size_t)std::min<uint64_t>(cap, s.size()));
        return s.size();
    } catch (const std::exception &) { return 0; }
}

int pdt_write_dcs_packets(const pdt_dcs_packet *packets, uint64_t n, int fd, uint64_t *bytes_written)
{
    if (bytes_written) *bytes_written = 0;
    if ((!packets && n) || fd < 0) return PDT_ERR_ARG;
    try {
        std::string s;
        dcs_text(packets, n, s);
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
