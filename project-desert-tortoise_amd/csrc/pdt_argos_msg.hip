// pdt_argos_msg.hip -- the ARGOS messages of a bit stream (pdt_argos_msg.h): the kernel that tests every bit for a head, the pass that
// applies the overlap rule and extracts the bodies (rule 0: k_argos_msgs, k_argos_finish; rule 1: k_argos_heads, k_argos_pick), their
// launch, the host restatement pdt_host_argos_messages and the text of the records.  A unit of its own, beside pdt_tone.hip.
#include <hip/hip_runtime.h>
#include <errno.h>
#include <stdio.h>
#include <unistd.h>
#include <algorithm>
#include <string>
#include <vector>

#include "../../include/pdt.h"
#include "pdt_argos_msg.h"

static_assert(sizeof(pdt_argos_msg) == sizeof(pdt::ArgosMsg) && sizeof(pdt_argos_msg) == 72, "pdt_argos_msg");
static_assert(sizeof(pdt::ArgosCtx) == 80, "the launch's table");
static_assert(sizeof(pdt_argos_cfg) == 16, "pdt_argos_cfg");
static_assert(pdt::ARGOS_RULE_FIRST == PDT_ARGOS_RULE_FIRST && pdt::ARGOS_RULE_BEST == PDT_ARGOS_RULE_BEST, "the rules' numbers");

namespace pdt {

// the context workgroup `block` of the grid belongs to: the last whose first tile is not behind it (first_tile ascends, [0] = 0)
__device__ __forceinline__ int argos_ctx_of(const ArgosCtx *__restrict__ table, int nctx, int block)
{
    int lo = 0, hi = nctx - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (table[mid].first_tile <= block) lo = mid; else hi = mid - 1;
    }
    return lo;
}

__device__ __forceinline__ long long argos_nbits(const ArgosCtx &c)
{
    if (c.bit_cap <= 0) return 0;
    const unsigned long long n = *c.nbits;
    return n < (unsigned long long)c.bit_cap ? (long long)n : c.bit_cap;
}

// One workgroup of 256 lanes per tile of ARGOS_MSG_TILE bits, all contexts of a call in one grid (a tile behind its context's device-side
// bit count returns at once: the grid is sized by what the buffers hold).  The wavefronts pack the tile's bytes into 64-bit words with
// __ballot -- bit l of a word = the bit at word * 64 + l -- and the 64 bits in front of the tile into a halo word (a head's test looks 27
// bits back).  Four lanes share a word: each tests sixteen positions for both polarities on the window shifted out of (halo or previous
// word, own word), the four 16-bit masks are joined by shuffles, and the word of the candidate bitmap goes to memory with the tile's
// number of heads.  No atomics, no list that could overflow; nothing depends on the order in which anything runs.
__global__ void __launch_bounds__(256) k_argos_msgs(const ArgosCtx *__restrict__ table, int nctx, int K)
{
    __shared__ unsigned long long words[1 + ARGOS_MSG_WORDS];
    __shared__ unsigned wsum[4];
    const ArgosCtx c = table[argos_ctx_of(table, nctx, (int)blockIdx.x)];
    const long long tile = (long long)blockIdx.x - c.first_tile, base = tile * ARGOS_MSG_TILE, nbits = argos_nbits(c);
    if (base >= nbits) return;
    const int t = (int)threadIdx.x, wave = t >> 6, lane = t & 63;
    for (int i = 0; i < ARGOS_MSG_WORDS / 4; i++) {
        const int w = 4 * i + wave;
        const long long idx = base + 64ll * w + lane;
        const unsigned long long m = __ballot(idx < nbits && c.bits[idx] != '0');
        if (lane == 0) words[1 + w] = m;
    }
    if (wave == 0) {
        const long long idx = base - 64 + lane;                               // (base < nbits: every such bit exists, or lies in front of the stream)
        const unsigned long long m = __ballot(idx >= 0 && c.bits[idx] != '0');
        if (lane == 0) words[0] = m;
    }
    __syncthreads();
    const int w = t >> 2, q = t & 3;
    const unsigned long long prev = words[w], cur = words[1 + w];
    unsigned long long mask = 0;
#pragma unroll 4
    for (int j = 0; j < 16; j++) {
        const int pos = 16 * q + j, s = 64 - (ARGOS_MSG_WINDOW - 1) + pos;    // the window's first bit in (prev, cur): 37 .. 100
        const long long e = base + 64ll * w + pos;
        const unsigned long long v = s < 64 ? (prev >> s) | (cur << (64 - s)) : cur >> (s - 64);
        if (e < nbits && argos_head((uint32_t)v & ((1u << ARGOS_MSG_WINDOW) - 1u), e, K)) mask |= 1ull << pos;
    }
    mask |= __shfl_xor(mask, 1);
    mask |= __shfl_xor(mask, 2);
    unsigned heads = 0;
    if (q == 0) {
        c.cand[tile * ARGOS_MSG_WORDS + w] = mask;
        heads = (unsigned)__popcll(mask);
    }
#pragma unroll
    for (int off = 32; off; off >>= 1) heads += __shfl_xor(heads, off);
    if (lane == 0) wsum[wave] = heads;
    __syncthreads();
    if (t == 0) c.tile_any[tile] = wsum[0] + wsum[1] + wsum[2] + wsum[3];
}

// One wavefront per context walks its candidates in ascending e: 64 tiles' counts at a time (a ballot finds the tiles with heads), a
// tile's 64 bitmap words at a time, a word's bits one by one -- every step uniform over the wavefront.  A head behind the last accepted
// body is accepted into a list in LDS; a full list, and the last one, is extracted a message per lane (body, flags, time source).
__global__ void __launch_bounds__(64) k_argos_finish(const ArgosCtx *__restrict__ table, int K)
{
    constexpr int LIST = 256;
    __shared__ long long acc_e[LIST];
    __shared__ unsigned acc_h[LIST];
    const ArgosCtx c = table[blockIdx.x];
    const long long nbits = argos_nbits(c), ntiles = (nbits + ARGOS_MSG_TILE - 1) / ARGOS_MSG_TILE;
    const int lane = (int)threadIdx.x;
    long long last_end = -1;
    unsigned found = 0;
    int pend = 0;                                                             // messages in the list: records found - pend .. found - 1
    auto extract = [&]() {
        __syncthreads();
        for (int k = lane; k < pend; k += 64) {
            const unsigned idx = found - (unsigned)pend + (unsigned)k;
            if (idx >= (unsigned)c.cap) continue;
            const long long e = acc_e[k];
            ArgosMsg *m = c.out + idx;
            argos_fill(c.bits, nbits, e, acc_h[k], m);
            const long long ts = c.bitsym ? c.symidx[c.bitsym[e]] : e;
            m->time_src = ts;
            m->time = (double)ts;
        }
        __syncthreads();
        pend = 0;
    };
    for (long long t0 = 0; t0 < ntiles; t0 += 64) {
        unsigned long long tiles = __ballot(t0 + lane < ntiles && c.tile_any[t0 + lane] != 0);
        while (tiles) {
            const long long tile = t0 + (__ffsll(tiles) - 1);
            tiles &= tiles - 1;
            const unsigned long long word = c.cand[tile * ARGOS_MSG_WORDS + lane];
            unsigned long long nz = __ballot(word != 0);
            while (nz) {
                const int w = __ffsll(nz) - 1;
                nz &= nz - 1;
                unsigned long long hw = __shfl(word, w);
                while (hw) {
                    const long long e = tile * ARGOS_MSG_TILE + 64ll * w + (__ffsll(hw) - 1);
                    hw &= hw - 1;
                    if (e - 12 <= last_end) continue;
                    const unsigned h = argos_head(argos_window(c.bits, e), e, K);
                    if (!h) continue;
                    last_end = argos_body_end(e, (int)(h & 15u));
                    if (lane == 0) {
                        acc_e[pend] = e;
                        acc_h[pend] = h;
                    }
                    pend++;
                    found++;
                    if (pend == LIST) extract();
                }
            }
        }
    }
    extract();
    if (lane == 0) *c.count = found;
}

// Rule 1's search: k_argos_msgs with the window of 29 bits (the 64-bit halo holds the 28 bits in front of a tile's first) and
// argos_head_best.  Candidate bitmap and per-tile counts as above, no list; the selection among the candidates is k_argos_pick's.
__global__ void __launch_bounds__(256) k_argos_heads(const ArgosCtx *__restrict__ table, int nctx, int K)
{
    __shared__ unsigned long long words[1 + ARGOS_MSG_WORDS];
    __shared__ unsigned wsum[4];
    const ArgosCtx c = table[argos_ctx_of(table, nctx, (int)blockIdx.x)];
    const long long tile = (long long)blockIdx.x - c.first_tile, base = tile * ARGOS_MSG_TILE, nbits = argos_nbits(c);
    if (base >= nbits) return;
    const int t = (int)threadIdx.x, wave = t >> 6, lane = t & 63;
    for (int i = 0; i < ARGOS_MSG_WORDS / 4; i++) {
        const int w = 4 * i + wave;
        const long long idx = base + 64ll * w + lane;
        const unsigned long long m = __ballot(idx < nbits && c.bits[idx < nbits ? idx : nbits - 1] != '0');
        if (lane == 0) words[1 + w] = m;
    }
    if (wave == 0) {
        const long long idx = base - 64 + lane;                               // (base < nbits: every such bit exists, or lies in front of the stream)
        const unsigned long long m = __ballot(idx >= 0 && c.bits[idx >= 0 ? idx : 0] != '0');
        if (lane == 0) words[0] = m;
    }
    __syncthreads();
    const int w = t >> 2, q = t & 3;
    const unsigned long long prev = words[w], cur = words[1 + w];
    unsigned long long mask = 0;
#pragma unroll 4
    for (int j = 0; j < 16; j++) {
        const int pos = 16 * q + j, s = 64 - (ARGOS_BEST_WINDOW - 1) + pos;   // the window's first bit in (prev, cur): 36 .. 99
        const long long e = base + 64ll * w + pos;
        const unsigned long long v = s < 64 ? (prev >> s) | (cur << (64 - s)) : cur >> (s - 64);
        if (e < nbits && argos_head_best((uint32_t)v & ((1u << ARGOS_BEST_WINDOW) - 1u), e, K)) mask |= 1ull << pos;
    }
    mask |= __shfl_xor(mask, 1);
    mask |= __shfl_xor(mask, 2);
    unsigned heads = 0;
    if (q == 0) {
        c.cand[tile * ARGOS_MSG_WORDS + w] = mask;
        heads = (unsigned)__popcll(mask);
    }
#pragma unroll
    for (int off = 32; off; off >>= 1) heads += __shfl_xor(heads, off);
    if (lane == 0) wsum[wave] = heads;
    __syncthreads();
    if (t == 0) c.tile_any[tile] = wsum[0] + wsum[1] + wsum[2] + wsum[3];
}

// Rule 1's selection.  One wavefront per context walks the candidate bitmap as k_argos_finish does.  The descriptors do not cost a
// round of dependent loads per candidate: a lane holds one of a tile's 64 bitmap words and reads the window of that word's first
// candidate itself, all 64 at once, so one round of loads serves a tile; only a word's further candidates (heads are seldom closer
// than 64 bits) are read one by one, 29 lanes and a ballot each.  The walk hands each descriptor on by shuffle, uniform over the
// wavefront.  Heads gather into a cluster in LDS (at most ARGOS_CLUSTER_MAX, four per lane once it is resolved).  A cluster of one
// head -- the usual case -- is decided at once.  Otherwise it is resolved by a wave-wide arg-max of the key (score, then the smaller
// index = the smaller e) over the live heads; every lane strikes those of its heads whose span overlaps the winner's, until none is
// live.  The winners go to the accepted list in ascending e (ballots rank them) and a full list, and the last one, is extracted a
// message per lane.  Control flow is uniform over the wavefront; per-lane work is predicated stores and selects.
__global__ void __launch_bounds__(64) k_argos_pick(const ArgosCtx *__restrict__ table, int K)
{
    constexpr int LIST = 256, PER = ARGOS_CLUSTER_MAX / 64;
    __shared__ long long acc_e[LIST], cl_e[ARGOS_CLUSTER_MAX];
    __shared__ unsigned acc_h[LIST], cl_h[ARGOS_CLUSTER_MAX];
    const ArgosCtx c = table[blockIdx.x];
    const long long nbits = argos_nbits(c), ntiles = (nbits + ARGOS_MSG_TILE - 1) / ARGOS_MSG_TILE;
    const int lane = (int)threadIdx.x;
    const unsigned long long below = (1ull << lane) - 1ull;
    long long prev_end = -1, cl_end = -1;                                     // the last span end accepted in the cluster before; the largest seen in this one
    long long one_e = 0;                                                      // the cluster's first head
    unsigned one_h = 0;
    int cl_n = 0;
    unsigned found = 0;
    int pend = 0;                                                             // messages in the list: records found - pend .. found - 1
    auto extract = [&]() {
        __syncthreads();
        for (int k = lane; k < pend; k += 64) {
            const unsigned idx = found - (unsigned)pend + (unsigned)k;
            if (idx >= (unsigned)c.cap) continue;
            const long long e = acc_e[k];
            const unsigned h = acc_h[k];
            ArgosMsg *m = c.out + idx;
            argos_fill(c.bits, nbits, e, h, m);
            m->reserved_ = argos_best_reserved(h);
            const long long ts = c.bitsym ? c.symidx[c.bitsym[e]] : e;
            m->time_src = ts;
            m->time = (double)ts;
        }
        __syncthreads();
        pend = 0;
    };
    auto resolve = [&]() {
        if (cl_n == 1) {                                                      // nothing to choose from: accepted unless the cluster before reaches it
            const bool take = one_e - 12 > prev_end;
            if (take && pend == LIST) extract();
            if (take && lane == 0) {
                acc_e[pend] = one_e;
                acc_h[pend] = one_h;
            }
            pend += take;
            found += take;
            prev_end = take ? argos_body_end(one_e, (int)(one_h & 15u)) : -1;
            cl_n = 0;
            cl_end = -1;
            return;
        }
        __syncthreads();
        long long e_[PER], end_[PER];
        unsigned h_[PER], key[PER];
#pragma unroll
        for (int j = 0; j < PER; j++) {
            const int i = lane + 64 * j, at = i < cl_n ? i : 0;               // (cl_n >= 1: entry 0 is there)
            e_[j] = cl_e[at];
            h_[j] = cl_h[at];
            end_[j] = argos_body_end(e_[j], (int)(h_[j] & 15u));
            key[j] = (i < cl_n && e_[j] - 12 > prev_end) ? ((argos_best_score(h_[j]) << 8) | (unsigned)(255 - i)) + 1u : 0u;
        }
        unsigned taken = 0;
        long long ends = -1;
        for (;;) {
            unsigned best = key[0];
#pragma unroll
            for (int j = 1; j < PER; j++) best = best > key[j] ? best : key[j];
#pragma unroll
            for (int off = 32; off; off >>= 1) {
                const unsigned o = (unsigned)__shfl_xor((int)best, off);
                best = best > o ? best : o;
            }
            if (!best) break;
            const int w = 255 - (int)((best - 1u) & 255u);
            const long long we = cl_e[w], wb = we - 12, wend = argos_body_end(we, (int)(cl_h[w] & 15u));
            ends = wend > ends ? wend : ends;
#pragma unroll
            for (int j = 0; j < PER; j++) {
                key[j] = (e_[j] - 12 <= wend && wb <= end_[j]) ? 0u : key[j];
                taken |= (unsigned)(w == lane + 64 * j) << j;
            }
        }
        unsigned long long bal[PER];
        int n = 0;
#pragma unroll
        for (int j = 0; j < PER; j++) {
            bal[j] = __ballot((taken >> j) & 1u);
            n += __popcll(bal[j]);
        }
        if (pend + n > LIST) extract();
        int at = pend;
#pragma unroll
        for (int j = 0; j < PER; j++) {
            if ((taken >> j) & 1u) {
                const int k = at + __popcll(bal[j] & below);
                acc_e[k] = e_[j];
                acc_h[k] = h_[j];
            }
            at += __popcll(bal[j]);
        }
        pend += n;
        found += (unsigned)n;
        prev_end = ends;
        cl_n = 0;
        cl_end = -1;
        __syncthreads();
    };
    for (long long t0 = 0; t0 < ntiles; t0 += 64) {
        unsigned long long tiles = __ballot(t0 + lane < ntiles && c.tile_any[t0 + lane < ntiles ? t0 + lane : 0] != 0);
        while (tiles) {
            const long long tile = t0 + (__ffsll(tiles) - 1);
            tiles &= tiles - 1;
            const unsigned long long word = c.cand[tile * ARGOS_MSG_WORDS + lane];
            // this lane's word's first candidate (a lane without one reads the window of the tile's first bit, which exists, and drops it)
            const long long own = tile * ARGOS_MSG_TILE + (word ? 64ll * lane + (__ffsll(word) - 1) : 0);
            const unsigned own_h = argos_head_best(argos_window_best(c.bits, own), own, K);
            unsigned long long nz = __ballot(word != 0);
            while (nz) {
                const int w = __ffsll(nz) - 1;
                nz &= nz - 1;
                unsigned long long hw = __shfl(word, w);
                unsigned h = (unsigned)__shfl((int)own_h, w);
                for (bool first = true; hw; first = false) {
                    const long long e = tile * ARGOS_MSG_TILE + 64ll * w + (__ffsll(hw) - 1);
                    hw &= hw - 1;
                    if (!first) {
                        const long long i = e - (ARGOS_BEST_WINDOW - 1) + lane;   // lanes 0 .. 28: the window's bits (e < nbits: the search tested it)
                        const bool in = lane < ARGOS_BEST_WINDOW && i >= 0;
                        h = argos_head_best((uint32_t)__ballot(in && c.bits[in ? i : 0] != '0'), e, K);
                    }
                    if (!h) continue;
                    if (cl_n && (e - 12 > cl_end || cl_n == ARGOS_CLUSTER_MAX)) resolve();
                    if (cl_n == 0) {
                        one_e = e;
                        one_h = h;
                    }
                    if (lane == 0) {
                        cl_e[cl_n] = e;
                        cl_h[cl_n] = h;
                    }
                    cl_n++;
                    const long long end = argos_body_end(e, (int)(h & 15u));
                    cl_end = end > cl_end ? end : cl_end;
                }
            }
        }
    }
    if (cl_n) resolve();
    extract();
    if (lane == 0) *c.count = found;
}

}  // namespace pdt

using namespace pdt;

namespace pdtrt {

// the two kernels over the nctx records of a table that is on the device; tiles: the grid of the first (the sum of the contexts' tiles).
// inner: NULL, or the one event recorded between the two (a profiled context times them apart: CallTimer; the caller records the
// first and the last).  rule 0: k_argos_msgs and k_argos_finish; rule 1: k_argos_heads and k_argos_pick
hipError_t argos_msgs_launch(hipStream_t st, const void *table_dev, int nctx, long long tiles, int K, int rule, hipEvent_t *inner)
{
    if (nctx < 1 || tiles < 0 || tiles > 0x7fffffffll || K < 0 || K > ARGOS_MSG_RUN_MAX) return hipErrorInvalidValue;
    if (rule != ARGOS_RULE_FIRST && rule != ARGOS_RULE_BEST) return hipErrorInvalidValue;
    const ArgosCtx *table = (const ArgosCtx *)table_dev;
    const bool best = rule == ARGOS_RULE_BEST;
    if (tiles) hipLaunchKernelGGL(best ? k_argos_heads : k_argos_msgs, dim3((unsigned)tiles), dim3(256), 0, st, table, nctx, K);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    if (inner && (e = hipEventRecord(inner[0], st)) != hipSuccess) return e;
    hipLaunchKernelGGL(best ? k_argos_pick : k_argos_finish, dim3((unsigned)nctx), dim3(64), 0, st, table, K);
    return hipGetLastError();
}

// cfg (NULL = the defaults) -> K and the rule; PDT_ERR_ARG for K outside 0 .. 15 or a rule other than 0 and 1
int argos_min_run(const pdt_argos_cfg *cfg, int *K, int *rule)
{
    *K = ARGOS_MSG_RUN_DEFAULT;
    *rule = ARGOS_RULE_FIRST;
    if (!cfg) return PDT_OK;
    if (cfg->rule != PDT_ARGOS_RULE_FIRST && cfg->rule != PDT_ARGOS_RULE_BEST) return PDT_ERR_ARG;
    *rule = cfg->rule;
    if (cfg->min_run < 0 || cfg->min_run > ARGOS_MSG_RUN_MAX) return PDT_ERR_ARG;
    if (cfg->min_run || (cfg->zero_mask & PDT_ARGOS_ZERO_MIN_RUN)) *K = cfg->min_run;
    return PDT_OK;
}

}  // namespace pdtrt

extern "C" {

int pdt_argos_msg_tile(void) { return ARGOS_MSG_TILE; }

int pdt_host_argos_messages(const uint8_t *bits, uint64_t nbits, const pdt_argos_cfg *cfg, pdt_argos_msg *out, int cap, int *count)
{
    int K, rule;
    if ((!bits && nbits) || nbits >= (1ull << 31) || cap < 0 || (!out && cap) || !count || pdtrt::argos_min_run(cfg, &K, &rule)) return PDT_ERR_ARG;
    *count = (int)(rule == ARGOS_RULE_BEST ? argos_host_messages_best : argos_host_messages)(bits, (long long)nbits, K, reinterpret_cast<ArgosMsg *>(out), cap);
    return PDT_OK;
}

// one line per complete message: "%.5f", "i" when inverted, " %d %05X" (blocks, id), " %02X" per data byte, "\n"
static void argos_text(const pdt_argos_msg *msgs, uint64_t n, std::string &s)
{
    char b[64];
    for (uint64_t i = 0; i < n; i++) {
        const pdt_argos_msg &m = msgs[i];
        if (!m.complete || m.blocks < 1 || m.blocks > 8) continue;
        snprintf(b, sizeof b, "%.5f%s %d %05X", m.time, m.inverted ? "i" : "", (int)m.blocks, (unsigned)m.id);
        s += b;
        for (int k = 0; k < 4 * m.blocks; k++) {
            snprintf(b, sizeof b, " %02X", (unsigned)m.data[k]);
            s += b;
        }
        s += '\n';
    }
}

uint64_t pdt_format_argos_messages(const pdt_argos_msg *msgs, uint64_t n, char *buf, uint64_t cap)
{
    if (!msgs && n) return 0;
    try {
        std::string s;
        argos_text(msgs, n, s);
        if (buf && cap) memcpy(buf, s.data(), (size_t)std::min<uint64_t>(cap, s.size()));
        return s.size();
    } catch (const std::exception &) { return 0; }
}

int pdt_write_argos_messages(const pdt_argos_msg *msgs, uint64_t n, int fd, uint64_t *bytes_written)
{
    if (bytes_written) *bytes_written = 0;
    if ((!msgs && n) || fd < 0) return PDT_ERR_ARG;
    try {
        std::string s;
        argos_text(msgs, n, s);
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
