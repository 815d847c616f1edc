// pdt_tip_sync.h -- a flywheel frame synchroniser for POES minor frames.  The reference's ByteSyncOnSyncword takes a minor
// frame only if all 19 bits of its sync word (or of the complement) are right, ignores sync words while a frame is open and accepts the
// first match it sees.  Minor frames come every 832 bits, so a sync word can be believed because its neighbours are where they should
// be, and a slot whose own sync word is damaged is still a frame if the slots around it say so.  There is no reference to be bit-exact
// against, so the rule is fixed here, once, for the kernels (pdt_tip_sync.hip) and their host restatement (pdt_host_tip_sync) alike:
//   b[i]      = bit i of the stream, 0 <= i < n: a byte of PDT_ST_BITS other than '0' is a one
//   S         = 1110110111100010000 (19 bits), F = 832
//   p         a position = the index of the bit that would complete a sync word (pdt_frame.bit_index), 18 <= p < n
//   dist+(p)  = the Hamming distance of b[p-18 .. p] to S;  dist-(p) = 19 - dist+(p)  (the reference's ring of '0' in front of the
//               stream is not modelled: no position below 18)
//   CANDIDATE c_s(p) <=> dist_s(p) <= E                              (E = max_errors, 0 .. 3, default 2)
//   SUPPORT   u_s(p) = the number of k in {-W .. -1, 1 .. W} with c_s(p + k F); a position outside [18, n) is no candidate
//                                                                     (W = window, 1 .. 8, default 2; exact multiples of F only)
//   HEAD      p is a head of polarity s <=> p + 813 < n (the whole frame is there) and
//               (c_s(p) and u_s(p) >= 1)  or  u_s(p) >= G            (G = fly, 2 .. 2 W, default 3: its own sync word may be damaged)
//   KEY       (u_s, c_s, -dist_s), compared lexicographically, larger first (tip_key below).  Both polarities heads at one p: the larger
//             key stands, at equal keys the upright one.  One record per p
//   OVERLAP   a head h is emitted <=> no other head g, emitted or not, beats it: |g - h| <= F - 4 and (key(g) > key(h) or the keys are
//             equal and g < h).  Not iterative, independent of any order; frames that overlap by up to three bits are both emitted
//   RECORD    a pdt_frame as the reference prints one: bytes[0] = 0xED, bytes[1] = 0xE2, bytes[2] = b[p+1 .. p+5] under three zero bits,
//             bytes[3 + j] = b[p+6+8j .. p+13+8j], MSB first, every data bit complemented when s = -; nbytes = 104, complete = 1,
//             inverted = (s = -); time_src and time those of a pdt_frame whose sync word completes at bit p.  Ascending bit_index.
//   INFO      sync_errors = dist_s(p), support = u_s(p), candidate = c_s(p) of the polarity that stands
// Emitted heads lie at least F - 3 = 829 bits apart (of two closer ones one beats the other): at most n / 829 + 1 records.
#pragma once
#include <stdint.h>
#include <string.h>
#include <vector>

namespace pdt {

constexpr int TIP_SYNC_TILE = 4096;                        // bits a workgroup packs and tests (pdt_tip_sync_tile())
constexpr int TIP_SYNC_WORDS = TIP_SYNC_TILE / 64;
constexpr int TIP_SYNC_F = 832, TIP_SYNC_LEN = 19, TIP_SYNC_BODY = 813, TIP_SYNC_REACH = TIP_SYNC_F - 4;
constexpr int TIP_SYNC_FW = TIP_SYNC_F / 64;               // F = 13 words of a bitmap exactly: the 64 positions of a word have their
static_assert(TIP_SYNC_FW * 64 == TIP_SYNC_F, "F");        // neighbours at +-k F in one word each, at word index +-13 k
constexpr int TIP_SYNC_E_DEFAULT = 2, TIP_SYNC_E_MAX = 3, TIP_SYNC_W_DEFAULT = 2, TIP_SYNC_W_MAX = 8, TIP_SYNC_G_DEFAULT = 3;
constexpr int TIP_SYNC_MIN_GAP = TIP_SYNC_F - 3;           // emitted heads are at least this far apart

// the sync word as a window reads it: bit j = its character j (bit 0 = b[p-18], bit 18 = b[p])
constexpr uint32_t tip_sync_word()
{
    const char s[TIP_SYNC_LEN + 1] = "1110110111100010000";
    uint32_t v = 0;
    for (int j = 0; j < TIP_SYNC_LEN; j++) v |= (uint32_t)(s[j] == '1') << j;
    return v;
}
constexpr uint32_t TIP_SYNC_WORD = tip_sync_word();
static_assert(TIP_SYNC_WORD == 0x47b7u, "the sync word");

struct TipSyncRule { int E, W, G; };

struct TipSyncRec {                 // (= pdt_frame of include/pdt.h)
    double time;
    int64_t bit_index, time_src;
    uint8_t inverted, nbytes, complete, pad;
    uint8_t bytes[104];
};

struct TipSyncInfo {                // (= pdt_tip_sync_info)
    uint8_t sync_errors, support, candidate, reserved;
};

struct TipSyncCtx {                 // one context of a launch: its bits and their count (device), its bitmaps, where its results go
    const unsigned char *bits;
    const unsigned long long *nbits;        // on the device: the chain leaves it there (DevScalars)
    const unsigned *bitsym;                 // bit -> symbol, symbol -> interpolated sample: the frames' time source; NULL: time_src = p
    const long long *symidx;
    unsigned long long *packed;             // bit i & 63 of word i >> 6 = b[i]; whole tiles, bits behind the stream are 0
    unsigned long long *cand[2];            // c_+ and c_-, laid out as packed
    unsigned long long *head[2];            // the heads of either polarity
    unsigned long long *emit;               // the heads no other head beats
    unsigned *tile_cnt, *tile_off;          // per tile: its emitted heads, and those of the tiles in front of it
    TipSyncRec *out;
    TipSyncInfo *info;
    unsigned *count;                        // frames found (may exceed cap: the first `cap` are written)
    long long bit_cap;                      // what the buffers hold: the count is read as min(*nbits, bit_cap)
    int cap;
    int first_tile;                         // the context's first workgroup in the launch's grid
};

// a head's key: (u, c, -dist) as one number
__host__ __device__ __forceinline__ unsigned tip_key(unsigned u, unsigned c, unsigned dist) { return (u << 6) | (c << 5) | (19u - dist); }

// g (key kg at position pg) beats h (kh at ph), the two within reach of each other
__host__ __device__ __forceinline__ bool tip_beats(unsigned kg, long long pg, unsigned kh, long long ph) { return kg > kh || (kg == kh && pg < ph); }

// the distance of a window (bit j = b[p-18+j]) to S, for the polarity s
__host__ __device__ __forceinline__ unsigned tip_dist(uint32_t window, int s)
{
    const unsigned d = (unsigned)__builtin_popcount((window ^ TIP_SYNC_WORD) & 0x7ffffu);
    return s ? 19u - d : d;
}

// payload byte t (0 .. 101) of the frame behind p from the characters: the first has five bits, the others eight
__host__ __device__ __forceinline__ uint8_t tip_byte(const unsigned char *bits, long long p, int t, unsigned inv)
{
    const int width = t ? 8 : 5;
    const long long b0 = p + 1 + (t ? 5 + 8ll * (t - 1) : 0);
    unsigned v = 0;
    for (int k = 0; k < width; k++) v = (v << 1) | ((unsigned)(bits[b0 + k] != '0') ^ inv);
    return (uint8_t)v;
}

// The rule on the host, straight from its text: out[0 .. min(found, cap)) with time_src = bit_index and time = its value; info may be
// NULL; returns found
inline long long tip_sync_host(const unsigned char *bits, long long n, TipSyncRule R, TipSyncRec *out, TipSyncInfo *info, long long cap)
{
    if (n < TIP_SYNC_LEN + TIP_SYNC_BODY) return 0;
    std::vector<uint8_t> dist((size_t)n, 0xff);                         // dist+(p), p >= 18
    uint32_t V = 0;
    for (long long p = 0; p < n; p++) {
        V = (V >> 1) | ((uint32_t)(bits[p] != '0') << (TIP_SYNC_LEN - 1));
        if (p >= TIP_SYNC_LEN - 1) dist[(size_t)p] = (uint8_t)tip_dist(V, 0);
    }
    auto dist_s = [&](long long p, int s) -> unsigned { return s ? 19u - dist[(size_t)p] : dist[(size_t)p]; };
    auto cand = [&](long long p, int s) -> bool { return p >= TIP_SYNC_LEN - 1 && p < n && dist_s(p, s) <= (unsigned)R.E; };
    struct Head { long long p; unsigned key; uint8_t inv, d, u, c; };
    std::vector<Head> heads;
    for (long long p = TIP_SYNC_LEN - 1; p + TIP_SYNC_BODY < n; p++) {
        bool have = false;
        Head h{};
        for (int s = 0; s < 2; s++) {
            unsigned u = 0;
            for (int k = 1; k <= R.W; k++) u += (unsigned)cand(p - (long long)k * TIP_SYNC_F, s) + (unsigned)cand(p + (long long)k * TIP_SYNC_F, s);
            const unsigned d = dist_s(p, s), c = d <= (unsigned)R.E;
            if (!((c && u >= 1) || u >= (unsigned)R.G)) continue;
            const unsigned key = tip_key(u, c, d);
            if (have && key <= h.key) continue;                         // (the upright one came first: it stands at equal keys)
            have = true;
            h = Head{ p, key, (uint8_t)s, (uint8_t)d, (uint8_t)u, (uint8_t)c };
        }
        if (have) heads.push_back(h);
    }
    long long found = 0;
    for (size_t i = 0; i < heads.size(); i++) {
        const Head &h = heads[i];
        bool beaten = false;
        for (size_t j = i; j-- > 0 && h.p - heads[j].p <= TIP_SYNC_REACH && !beaten;) beaten = tip_beats(heads[j].key, heads[j].p, h.key, h.p);
        for (size_t j = i + 1; j < heads.size() && heads[j].p - h.p <= TIP_SYNC_REACH && !beaten; j++) beaten = tip_beats(heads[j].key, heads[j].p, h.key, h.p);
        if (beaten) continue;
        if (found < cap) {
            TipSyncRec *r = &out[found];
            memset(r, 0, sizeof *r);
            r->time = (double)h.p;
            r->bit_index = h.p;
            r->time_src = h.p;
            r->inverted = h.inv;
            r->nbytes = 104;
            r->complete = 1;
            r->bytes[0] = 0xED;
            r->bytes[1] = 0xE2;
            for (int t = 0; t < 102; t++) r->bytes[2 + t] = tip_byte(bits, h.p, t, h.inv);
            if (info) info[found] = TipSyncInfo{ h.d, h.u, h.c, 0 };
        }
        found++;
    }
    return found;
}

}  // namespace pdt
