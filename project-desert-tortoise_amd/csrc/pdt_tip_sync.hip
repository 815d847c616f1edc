// pdt_tip_sync.hip -- the flywheel frame synchroniser of POES bit streams (pdt_tip_sync.h): the kernels that pack the bits and test every
// position for a candidate (k_tip_cand), add the candidates of the neighbouring slots bit-sliced and mark the heads (k_tip_heads), strike
// the heads another one beats (k_tip_pick), scan the tiles' counts (k_tip_scan) and write the records in ascending order (k_tip_pack),
// their launch, the cfg's rule and the host restatement pdt_host_tip_sync.  A unit of its own, beside pdt_argos_msg.hip.
#include <hip/hip_runtime.h>
#include <exception>

#include "../../include/pdt.h"
#include "pdt_tip_sync.h"

static_assert(sizeof(pdt_frame) == sizeof(pdt::TipSyncRec) && sizeof(pdt_frame) == 136, "pdt_frame");
static_assert(sizeof(pdt_tip_sync_info) == sizeof(pdt::TipSyncInfo) && sizeof(pdt_tip_sync_info) == 4, "pdt_tip_sync_info");
static_assert(sizeof(pdt_tip_sync_cfg) == 16, "pdt_tip_sync_cfg");
static_assert(sizeof(pdt::TipSyncCtx) == 136, "the launch's table");

namespace pdt {

// the context workgroup `block` of the grid belongs to: the last whose first tile is not behind it (first_tile ascends, [0] = 0)
__device__ __forceinline__ int tip_ctx_of(const TipSyncCtx *__restrict__ table, int nctx, int block)
{
    int lo = 0, hi = nctx - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (table[mid].first_tile <= block) lo = mid; else hi = mid - 1;
    }
    return lo;
}

__device__ __forceinline__ long long tip_nbits(const TipSyncCtx &c)
{
    if (c.bit_cap <= 0) return 0;
    const unsigned long long n = *c.nbits;
    return n < (unsigned long long)c.bit_cap ? (long long)n : c.bit_cap;
}

// word `wi` of a bitmap of the context: 0 in front of the stream and behind its last tile (the tiles behind the stream are never written)
__device__ __forceinline__ unsigned long long tip_word(const unsigned long long *__restrict__ map, long long wi, long long nbits)
{
    return wi >= 0 && wi * 64 < nbits ? map[wi] : 0ull;
}

__device__ __forceinline__ unsigned tip_bit(const unsigned long long *__restrict__ map, long long q, long long nbits)
{
    return q >= 0 && q < nbits ? (unsigned)(map[q >> 6] >> (q & 63)) & 1u : 0u;
}

// the 19 bits up to p (18 <= p < nbits) out of the packed words: bit j = b[p - 18 + j]
__device__ __forceinline__ uint32_t tip_window(const unsigned long long *__restrict__ packed, long long p)
{
    const long long first = p - (TIP_SYNC_LEN - 1);
    const int sh = (int)(first & 63);
    unsigned long long v = packed[first >> 6] >> sh;
    if (sh > 64 - TIP_SYNC_LEN) v |= packed[(first >> 6) + 1] << (64 - sh);       // (p lies in that word)
    return (uint32_t)v & 0x7ffffu;
}

// One workgroup of 256 lanes per tile of TIP_SYNC_TILE bits, all contexts of a call in one grid (a tile behind its context's device-side
// bit count returns at once).  The wavefronts pack the tile's bytes into 64-bit words with __ballot and the 64 bits in front of the tile
// into a halo word (a test looks 18 bits back).  Four lanes share a word: each tests sixteen positions for both polarities -- one
// popcount against S -- the four 16-bit masks are joined by shuffles, and the packed word and the two candidate words go to memory.
__global__ void __launch_bounds__(256) k_tip_cand(const TipSyncCtx *__restrict__ table, int nctx, TipSyncRule R)
{
    __shared__ unsigned long long words[1 + TIP_SYNC_WORDS];
    const TipSyncCtx c = table[tip_ctx_of(table, nctx, (int)blockIdx.x)];
    const long long tile = (long long)blockIdx.x - c.first_tile, base = tile * TIP_SYNC_TILE, nbits = tip_nbits(c);
    if (base >= nbits) return;
    const int t = (int)threadIdx.x, wave = t >> 6, lane = t & 63;
    for (int i = 0; i < TIP_SYNC_WORDS / 4; i++) {
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
    unsigned long long up = 0, dn = 0;
#pragma unroll 4
    for (int j = 0; j < 16; j++) {
        const int pos = 16 * q + j, s = 64 - (TIP_SYNC_LEN - 1) + pos;        // the window's first bit in (prev, cur): 46 .. 109
        const long long p = base + 64ll * w + pos;
        const unsigned long long v = s < 64 ? (prev >> s) | (cur << (64 - s)) : cur >> (s - 64);
        const unsigned d = tip_dist((uint32_t)v & 0x7ffffu, 0);
        const bool in = p >= TIP_SYNC_LEN - 1 && p < nbits;
        if (in && d <= (unsigned)R.E) up |= 1ull << pos;
        if (in && 19u - d <= (unsigned)R.E) dn |= 1ull << pos;
    }
    up |= __shfl_xor(up, 1);
    up |= __shfl_xor(up, 2);
    dn |= __shfl_xor(dn, 1);
    dn |= __shfl_xor(dn, 2);
    if (q == 0) {
        const long long at = tile * TIP_SYNC_WORDS + w;
        c.packed[at] = cur;
        c.cand[0][at] = up;
        c.cand[1][at] = dn;
    }
}

// One wavefront per tile, a lane per word of the bitmaps.  F is 13 words exactly, so the 64 positions of a word find the candidates of
// their slots at +-k F in the word at +-13 k: the 2 W words are added bit-sliced into five planes (u <= 16), u >= 1 is the planes' OR and
// u >= G a bit-sliced comparison.  Every position is tested -- a flywheel head is by definition no candidate itself.
__global__ void __launch_bounds__(64) k_tip_heads(const TipSyncCtx *__restrict__ table, int nctx, TipSyncRule R)
{
    const TipSyncCtx c = table[tip_ctx_of(table, nctx, (int)blockIdx.x)];
    const long long tile = (long long)blockIdx.x - c.first_tile, base = tile * TIP_SYNC_TILE, nbits = tip_nbits(c);
    if (base >= nbits) return;
    const long long gw = tile * TIP_SYNC_WORDS + (int)threadIdx.x, p0 = gw * 64;
    // the positions of this word that can be heads: 18 <= p and p + 813 < nbits
    const long long lo = TIP_SYNC_LEN - 1 - p0 > 0 ? TIP_SYNC_LEN - 1 - p0 : 0, hi = nbits - 1 - TIP_SYNC_BODY - p0 < 63 ? nbits - 1 - TIP_SYNC_BODY - p0 : 63;
    unsigned long long span = 0;
    if (hi >= lo) span = (hi == 63 ? ~0ull : (1ull << (hi + 1)) - 1ull) & ~((1ull << lo) - 1ull);
    for (int s = 0; s < 2; s++) {
        unsigned long long pl[5] = { 0, 0, 0, 0, 0 };
        for (int k = 1; k <= R.W; k++) {
#pragma unroll
            for (int sg = -1; sg <= 1; sg += 2) {
                unsigned long long carry = tip_word(c.cand[s], gw + (long long)sg * k * TIP_SYNC_FW, nbits);
#pragma unroll
                for (int i = 0; i < 5; i++) {
                    const unsigned long long both = pl[i] & carry;
                    pl[i] ^= carry;
                    carry = both;
                }
            }
        }
        const unsigned long long ge1 = pl[0] | pl[1] | pl[2] | pl[3] | pl[4];
        unsigned long long gt = 0, eq = ~0ull;                                // u > G, u == G on the planes looked at so far
#pragma unroll
        for (int i = 4; i >= 0; i--) {
            const unsigned long long g = (R.G >> i) & 1 ? ~0ull : 0ull;
            gt |= eq & pl[i] & ~g;
            eq &= ~(pl[i] ^ g);
        }
        c.head[s][gw] = span & ((c.cand[s][gw] & ge1) | gt | eq);
    }
}

// what stands at the head position p: its key, and through `o` (when not NULL) polarity, distance, support and candidate bit.  The support
// is counted by the rule's text, bit by bit -- heads are rare, about one per 832 bits
struct TipStand { unsigned inv, d, u, c; };
__device__ __forceinline__ unsigned tip_stands(const TipSyncCtx &c, long long nbits, long long p, TipSyncRule R, TipStand *o)
{
    const uint32_t win = tip_window(c.packed, p);
    const unsigned hp = tip_bit(c.head[0], p, nbits), hm = tip_bit(c.head[1], p, nbits);
    unsigned key[2] = { 0, 0 }, us[2] = { 0, 0 };
    for (int s = 0; s < 2; s++) {
        if (!(s ? hm : hp)) continue;
        unsigned u = 0;
        for (int k = 1; k <= R.W; k++)
            u += tip_bit(c.cand[s], p - (long long)k * TIP_SYNC_F, nbits) + tip_bit(c.cand[s], p + (long long)k * TIP_SYNC_F, nbits);
        const unsigned d = tip_dist(win, s);
        us[s] = u;
        key[s] = tip_key(u, d <= (unsigned)R.E, d);
    }
    const int s = hm && (!hp || key[1] > key[0]) ? 1 : 0;                     // at equal keys the upright one stands
    if (o) {
        const unsigned d = tip_dist(win, s);
        *o = TipStand{ (unsigned)s, d, us[s], (unsigned)(d <= (unsigned)R.E) };
    }
    return key[s];
}

// One wavefront per tile, a lane per word of the head bitmaps.  A lane walks the heads of its word (they are rare); for each it looks
// through the head words within F - 4 bits on either side and forms the key of every other head there.  A head none of them beats gets
// its bit in the emit bitmap; the tile's number of them goes to tile_cnt.  Nothing depends on an order: every head is judged against the
// heads themselves, not against what was emitted.
__global__ void __launch_bounds__(64) k_tip_pick(const TipSyncCtx *__restrict__ table, int nctx, TipSyncRule R)
{
    const TipSyncCtx c = table[tip_ctx_of(table, nctx, (int)blockIdx.x)];
    const long long tile = (long long)blockIdx.x - c.first_tile, base = tile * TIP_SYNC_TILE, nbits = tip_nbits(c);
    if (base >= nbits) return;
    const int lane = (int)threadIdx.x;
    const long long gw = tile * TIP_SYNC_WORDS + lane;
    unsigned long long mine = c.head[0][gw] | c.head[1][gw], emit = 0;
    while (mine) {
        const int bit = __ffsll(mine) - 1;
        mine &= mine - 1;
        const long long p = gw * 64 + bit, first = p - TIP_SYNC_REACH, last = p + TIP_SYNC_REACH;
        const unsigned key = tip_stands(c, nbits, p, R, nullptr);
        bool beaten = false;
        for (long long wi = first >> 6; wi <= (last >> 6) && !beaten; wi++) {      // (first may be negative: >> rounds down, tip_word gives 0)
            unsigned long long m = tip_word(c.head[0], wi, nbits) | tip_word(c.head[1], wi, nbits);
            if (wi == (first >> 6)) m &= ~0ull << (first & 63);
            if (wi == (last >> 6)) m &= ~0ull >> (63 - (last & 63));
            if (wi == gw) m &= ~(1ull << bit);
            while (m && !beaten) {
                const long long g = wi * 64 + (__ffsll(m) - 1);
                m &= m - 1;
                beaten = tip_beats(tip_stands(c, nbits, g, R, nullptr), g, key, p);
            }
        }
        if (!beaten) emit |= 1ull << bit;
    }
    c.emit[gw] = emit;
    unsigned n = (unsigned)__popcll(emit);
#pragma unroll
    for (int off = 32; off; off >>= 1) n += __shfl_xor(n, off);
    if (lane == 0) c.tile_cnt[tile] = n;
}

// One workgroup per context: the exclusive scan of its tiles' counts, 256 tiles at a time, and the total -- the frames found
__global__ void __launch_bounds__(256) k_tip_scan(const TipSyncCtx *__restrict__ table)
{
    __shared__ unsigned sc[2][256];
    const TipSyncCtx c = table[blockIdx.x];
    const long long nbits = tip_nbits(c), ntiles = (nbits + TIP_SYNC_TILE - 1) / TIP_SYNC_TILE;
    const int t = (int)threadIdx.x;
    unsigned running = 0;
    for (long long t0 = 0; t0 < ntiles; t0 += 256) {
        const unsigned v = t0 + t < ntiles ? c.tile_cnt[t0 + t] : 0u;
        int cur = 0;
        sc[0][t] = v;
        __syncthreads();
        for (int off = 1; off < 256; off <<= 1) {
            sc[cur ^ 1][t] = sc[cur][t] + (t >= off ? sc[cur][t - off] : 0u);
            cur ^= 1;
            __syncthreads();
        }
        if (t0 + t < ntiles) c.tile_off[t0 + t] = running + sc[cur][t] - v;
        running += sc[cur][255];
        __syncthreads();
    }
    if (t == 0) *c.count = running;
}

// One workgroup of 128 lanes per tile: the tile's emitted heads in ascending p (every lane walks the 64 emit words alike), record
// tile_off + rank each, written while it is below cap -- lane t packs payload byte t from the characters as k_frame_pack does, lane 127
// the fixed fields, the time source and the info record.
__global__ void __launch_bounds__(128) k_tip_pack(const TipSyncCtx *__restrict__ table, int nctx, TipSyncRule R)
{
    __shared__ unsigned long long words[TIP_SYNC_WORDS];
    const TipSyncCtx c = table[tip_ctx_of(table, nctx, (int)blockIdx.x)];
    const long long tile = (long long)blockIdx.x - c.first_tile, base = tile * TIP_SYNC_TILE, nbits = tip_nbits(c);
    if (base >= nbits) return;
    const int t = (int)threadIdx.x;
    if (t < TIP_SYNC_WORDS) words[t] = c.emit[tile * TIP_SYNC_WORDS + t];
    __syncthreads();
    unsigned at = c.tile_off[tile];
    for (int w = 0; w < TIP_SYNC_WORDS; w++) {
        unsigned long long m = words[w];
        while (m) {
            const long long p = base + 64ll * w + (__ffsll(m) - 1);           // (a head: p + 813 < nbits, every bit read below exists)
            m &= m - 1;
            const unsigned idx = at++;
            if (idx >= (unsigned)c.cap) continue;
            TipStand st;
            (void)tip_stands(c, nbits, p, R, &st);
            TipSyncRec *r = c.out + idx;
            if (t < 102) r->bytes[2 + t] = tip_byte(c.bits, p, t, st.inv);
            else if (t < 106) reinterpret_cast<unsigned char *>(r)[sizeof(TipSyncRec) - 106 + t] = 0;   // (the record's four bytes of padding: records compare as bytes)
            if (t == 127) {
                const long long ts = c.bitsym ? c.symidx[c.bitsym[p]] : p;
                r->time = (double)ts;
                r->bit_index = p;
                r->time_src = ts;
                r->inverted = (uint8_t)st.inv;
                r->nbytes = 104;
                r->complete = 1;
                r->pad = 0;
                r->bytes[0] = 0xED;
                r->bytes[1] = 0xE2;
                c.info[idx] = TipSyncInfo{ (uint8_t)st.d, (uint8_t)st.u, (uint8_t)st.c, 0 };
            }
        }
    }
}

}  // namespace pdt

using namespace pdt;

namespace pdtrt {

extern const char *const tip_sync_kernel_names[5] = { "k_tip_cand", "k_tip_heads", "k_tip_pick", "k_tip_scan", "k_tip_pack" };

// the five kernels over the nctx records of a table that is on the device; tiles: the grid of the tiled ones (the sum of the contexts'
// tiles).  inner: NULL, or the four events recorded between the kernels (a profiled context times them apart under
// tip_sync_kernel_names: CallTimer; the caller records the first and the last)
hipError_t tip_sync_launch(hipStream_t st, const void *table_dev, int nctx, long long tiles, TipSyncRule R, hipEvent_t *inner)
{
    if (nctx < 1 || tiles < 0 || tiles > 0x7fffffffll) return hipErrorInvalidValue;
    const TipSyncCtx *table = (const TipSyncCtx *)table_dev;
    hipError_t e;
    auto mark = [&](int k) -> hipError_t { return inner ? hipEventRecord(inner[k], st) : hipSuccess; };
    if (tiles) hipLaunchKernelGGL(k_tip_cand, dim3((unsigned)tiles), dim3(256), 0, st, table, nctx, R);
    if ((e = hipGetLastError()) != hipSuccess || (e = mark(0)) != hipSuccess) return e;
    if (tiles) hipLaunchKernelGGL(k_tip_heads, dim3((unsigned)tiles), dim3(64), 0, st, table, nctx, R);
    if ((e = hipGetLastError()) != hipSuccess || (e = mark(1)) != hipSuccess) return e;
    if (tiles) hipLaunchKernelGGL(k_tip_pick, dim3((unsigned)tiles), dim3(64), 0, st, table, nctx, R);
    if ((e = hipGetLastError()) != hipSuccess || (e = mark(2)) != hipSuccess) return e;
    hipLaunchKernelGGL(k_tip_scan, dim3((unsigned)nctx), dim3(256), 0, st, table);
    if ((e = hipGetLastError()) != hipSuccess || (e = mark(3)) != hipSuccess) return e;
    if (tiles) hipLaunchKernelGGL(k_tip_pack, dim3((unsigned)tiles), dim3(128), 0, st, table, nctx, R);
    return hipGetLastError();
}

// cfg (NULL = the defaults) -> E, W, G; PDT_ERR_ARG for a value out of range
int tip_sync_rule(const pdt_tip_sync_cfg *cfg, TipSyncRule *R)
{
    *R = TipSyncRule{ TIP_SYNC_E_DEFAULT, TIP_SYNC_W_DEFAULT, TIP_SYNC_G_DEFAULT };
    if (!cfg) return PDT_OK;
    if (cfg->max_errors < 0 || cfg->max_errors > TIP_SYNC_E_MAX) return PDT_ERR_ARG;
    if (cfg->max_errors || (cfg->zero_mask & PDT_TIP_SYNC_ZERO_MAX_ERRORS)) R->E = cfg->max_errors;
    if (cfg->window < 0 || cfg->window > TIP_SYNC_W_MAX) return PDT_ERR_ARG;
    if (cfg->window) R->W = cfg->window;
    if (cfg->fly < 0 || cfg->fly == 1) return PDT_ERR_ARG;
    if (cfg->fly) R->G = cfg->fly;
    if (R->G < 2 || R->G > 2 * R->W) return PDT_ERR_ARG;
    return PDT_OK;
}

}  // namespace pdtrt

extern "C" {

int pdt_tip_sync_tile(void) { return TIP_SYNC_TILE; }

int pdt_host_tip_sync(const uint8_t *bits, uint64_t nbits, const pdt_tip_sync_cfg *cfg, pdt_frame *out, pdt_tip_sync_info *info, int cap, int *count)
{
    TipSyncRule R;
    if ((!bits && nbits) || nbits >= (1ull << 31) || cap < 0 || (!out && cap) || !count || pdtrt::tip_sync_rule(cfg, &R)) return PDT_ERR_ARG;
    try {
        *count = (int)tip_sync_host(bits, (long long)nbits, R, reinterpret_cast<TipSyncRec *>(out), reinterpret_cast<TipSyncInfo *>(info), cap);
    } catch (const std::exception &) { return PDT_ERR_NOMEM; }
    return PDT_OK;
}

}  // extern "C"
