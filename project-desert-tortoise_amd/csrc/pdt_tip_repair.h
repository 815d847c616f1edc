// pdt_tip_repair.h -- repair of failed TIP parity groups from the soft bit values.  The flywheel (pdt_tip_sync.h) places the
// minor frames of a weak pass; what it hands out are hard decisions, and pdt_tip_check only REPORTS the five even-parity groups of a frame.
// Where a group's parity is odd, complementing its least reliable bit (Wagner's rule for a single-parity code) is the most likely
// correction.  There is no reference to be bit-exact against, so the rule is fixed here, once, for the kernel (pdt_tip_repair.hip) and
// its host restatement (pdt_host_tip_repair) alike:
//   input     pdt_frame records as pdt_tip_sync / pdt_ffp_frames give them, and a stream of n float32 soft values: value k belongs to
//             bit k of the stream the records were found in (pdt_ffp_read's soft)
//   CHECKED   a record is checked <=> complete == 1 and nbytes == 104 and 18 <= bit_index and bit_index + 813 < n.  Any other record is
//             left as it is and marked skipped
//   BITS      frame bit j, 0 <= j < 832, is bit 7 - (j & 7) of bytes[j >> 3]; its soft value is soft[bit_index - 18 + j]
//   GROUPS    k_tip_check's, unchanged: group g = 0 .. 4 covers frame bits 16 + 136 g .. 151 + 136 g (bytes 2 + 17 g .. 18 + 17 g) and
//             its parity bit, frame bit 826 + g (bit 5 - g of bytes[103]).  The group FAILS when the number of ones among these 137 bits
//             OF THE RECORD is odd; the record of an inverted head is already complemented back, so polarity plays no part
//   CANDIDATE the group's bits that came from the stream.  In group 0 frame bits 16, 17 and 18 are the sync word's last three bits, which
//             k_tip_pack writes as zeros: they count toward the parity but are never candidates -- 134 candidates in group 0, 137 in
//             the others
//   r(k)      the uint32 bit pattern of |soft[k]|: a NaN counts as 0, -0 as 0, Inf sorts above every finite value
//   KEY       of the candidate at frame bit j: (uint64) r << 16 | j
//   REPAIR    in a failing group the candidate with the smallest key is complemented in the record: ties go to the earlier bit, a data
//             bit goes before the parity bit.  Nothing else changes -- not time, bit_index, time_src, inverted or bytes 0 - 1
//   INFO      per record: status (1 checked, 0 skipped); failed, bit g set where group g failed BEFORE the repair; pos[g] = the frame bit
//             complemented in group g, or 0xFFFF; least[g] and next[g] = the floats whose bit patterns are the r of the smallest and the
//             second smallest key of group g, filled whether or not the group failed (a repair is judged by its margin).  A skipped
//             record: failed 0, pos 0xFFFF, least and next 0
//   SUMMARY   records checked, records skipped, records with a failing group, groups repaired
// After the repair every group of a checked record passes BY CONSTRUCTION: -q and pdt_tip_check_records on repaired records say nothing,
// and `failed` is the parity record to keep.  A group with two wrong bits passes as it is, one with three is made worse: the rule helps
// while single errors dominate (DESIGN 4.20's table says where that ends).
#pragma once
#include <stdint.h>
#include <string.h>

#ifndef __host__
#define __host__
#define __device__
#endif

namespace pdt {

constexpr int TIP_REPAIR_GROUPS = 5, TIP_REPAIR_DATA = 136, TIP_REPAIR_CAND = 137;   // a group: 136 data bits and the parity bit
constexpr int TIP_REPAIR_FIRST = 16, TIP_REPAIR_PARITY = 826, TIP_REPAIR_BODY = 813, TIP_REPAIR_LEAD = 18;
constexpr int TIP_REPAIR_BYTES = 28;                       // offsetof(pdt_frame, bytes)
constexpr uint16_t TIP_REPAIR_NONE = 0xFFFF;
constexpr uint64_t TIP_REPAIR_NOKEY = ~0ull;               // above every key: r < 2^32, j < 2^16

struct TipRepairRec {               // (= pdt_frame of include/pdt.h)
    double time;
    int64_t bit_index, time_src;
    uint8_t inverted, nbytes, complete, pad;
    uint8_t bytes[104];
};

struct TipRepairInfo {              // (= pdt_tip_repair_info)
    uint8_t status, failed;
    uint16_t pos[TIP_REPAIR_GROUPS];
    float least[TIP_REPAIR_GROUPS], next[TIP_REPAIR_GROUPS];
};

struct TipRepairSummary {           // (= pdt_tip_repair_summary)
    uint64_t checked, skipped, failing, repaired;
};

struct TipRepairPair { uint64_t lo, hi; };                 // the two smallest keys of a set, lo < hi (NOKEY: there is none)

// a record is checked against a stream of n soft values
__host__ __device__ inline bool tip_repair_checked(uint8_t complete, uint8_t nbytes, int64_t bit_index, int64_t n)
{
    return complete == 1 && nbytes == 104 && bit_index >= TIP_REPAIR_LEAD && bit_index < n - TIP_REPAIR_BODY;
}

// r: the bit pattern of |x|, a NaN as 0 (-0 and +0 are 0 already)
__host__ __device__ inline uint32_t tip_repair_rel(uint32_t pattern)
{
    const uint32_t a = pattern & 0x7fffffffu;
    return a > 0x7f800000u ? 0u : a;
}

__host__ __device__ inline uint64_t tip_repair_key(uint32_t r, int j) { return ((uint64_t)r << 16) | (uint64_t)(unsigned)j; }

// candidate c = 0 .. 136 of group g: its frame bit, or -1 for group 0's three sync bits
__host__ __device__ inline int tip_repair_cand(int g, int c)
{
    if (c == TIP_REPAIR_DATA) return TIP_REPAIR_PARITY + g;
    const int j = TIP_REPAIR_FIRST + TIP_REPAIR_DATA * g + c;
    return j <= TIP_REPAIR_LEAD ? -1 : j;
}

// the two smallest of the union of two sets whose keys are all different
__host__ __device__ inline TipRepairPair tip_repair_merge(TipRepairPair a, TipRepairPair b)
{
    const uint64_t lo = a.lo < b.lo ? a.lo : b.lo, mid = a.lo < b.lo ? b.lo : a.lo, up = a.hi < b.hi ? a.hi : b.hi;
    return TipRepairPair{ lo, mid < up ? mid : up };
}

// a lane's share of group g: candidates lane, lane + 64 and lane + 128; soft0 = the soft value of frame bit 0 (soft + bit_index - 18)
__host__ __device__ inline TipRepairPair tip_repair_lane(const float *soft0, int g, int lane)
{
    TipRepairPair p{ TIP_REPAIR_NOKEY, TIP_REPAIR_NOKEY };
    for (int c = lane; c < TIP_REPAIR_CAND; c += 64) {
        const int j = tip_repair_cand(g, c);
        if (j < 0) continue;
        uint32_t w;
        memcpy(&w, soft0 + j, sizeof w);
        p = tip_repair_merge(p, TipRepairPair{ tip_repair_key(tip_repair_rel(w), j), TIP_REPAIR_NOKEY });
    }
    return p;
}

// the parity of byte t = 0 .. 16 of group g, and of its parity bit
__host__ __device__ inline unsigned tip_repair_byte_odd(const uint8_t *bytes, int g, int t) { return (unsigned)__builtin_popcount(bytes[2 + 17 * g + t]) & 1u; }
__host__ __device__ inline unsigned tip_repair_parity_bit(const uint8_t *bytes, int g) { return (unsigned)(bytes[103] >> (5 - g)) & 1u; }

// frame bit j as a complement of the record's aligned 32-bit words (little endian): the word's index and the mask.  bytes[103] is the
// top byte of word 32, where up to five groups meet: one XOR of a word, never a read-modify-write of a byte
__host__ __device__ inline int tip_repair_word(int j) { return (TIP_REPAIR_BYTES + (j >> 3)) >> 2; }
__host__ __device__ inline uint32_t tip_repair_mask(int j) { return (uint32_t)(0x80u >> (j & 7)) << (8 * ((TIP_REPAIR_BYTES + (j >> 3)) & 3)); }

__host__ __device__ inline float tip_repair_float(uint64_t key)
{
    const uint32_t w = key == TIP_REPAIR_NOKEY ? 0u : (uint32_t)(key >> 16);
    float f;
    memcpy(&f, &w, sizeof f);
    return f;
}

// The rule on the host, straight from its text: recs[0 .. count) repaired in place, info (may be NULL) and *sum filled
inline void tip_repair_host(const float *soft, int64_t n, TipRepairRec *recs, uint64_t count, TipRepairInfo *info, TipRepairSummary *sum)
{
    memset(sum, 0, sizeof *sum);
    for (uint64_t f = 0; f < count; f++) {
        TipRepairRec &r = recs[f];
        TipRepairInfo I;
        memset(&I, 0, sizeof I);
        for (int g = 0; g < TIP_REPAIR_GROUPS; g++) I.pos[g] = TIP_REPAIR_NONE;
        if (!tip_repair_checked(r.complete, r.nbytes, r.bit_index, n)) {
            sum->skipped++;
            if (info) info[f] = I;
            continue;
        }
        I.status = 1;
        sum->checked++;
        const float *soft0 = soft + (r.bit_index - TIP_REPAIR_LEAD);
        int flips[TIP_REPAIR_GROUPS], nflips = 0;
        for (int g = 0; g < TIP_REPAIR_GROUPS; g++) {
            unsigned ones = 0;
            for (int j = TIP_REPAIR_FIRST + TIP_REPAIR_DATA * g; j < TIP_REPAIR_FIRST + TIP_REPAIR_DATA * (g + 1); j++) ones += (r.bytes[j >> 3] >> (7 - (j & 7))) & 1u;
            ones += (r.bytes[103] >> (5 - g)) & 1u;
            uint64_t lo = TIP_REPAIR_NOKEY, hi = TIP_REPAIR_NOKEY;
            for (int c = 0; c < TIP_REPAIR_CAND; c++) {
                const int j = c < TIP_REPAIR_DATA ? TIP_REPAIR_FIRST + TIP_REPAIR_DATA * g + c : TIP_REPAIR_PARITY + g;
                if (j <= TIP_REPAIR_LEAD) continue;
                uint32_t w;
                memcpy(&w, soft0 + j, sizeof w);
                w &= 0x7fffffffu;
                if (w > 0x7f800000u) w = 0;
                const uint64_t key = ((uint64_t)w << 16) | (uint64_t)j;
                if (key < lo) { hi = lo; lo = key; }
                else if (key < hi) hi = key;
            }
            I.least[g] = tip_repair_float(lo);
            I.next[g] = tip_repair_float(hi);
            if (ones & 1u) {
                I.failed |= (uint8_t)(1u << g);
                I.pos[g] = (uint16_t)(lo & 0xffffu);
                flips[nflips++] = (int)(lo & 0xffffu);
            }
        }
        for (int k = 0; k < nflips; k++) r.bytes[flips[k] >> 3] ^= (uint8_t)(0x80u >> (flips[k] & 7));
        if (nflips) sum->failing++;
        sum->repaired += (uint64_t)nflips;
        if (info) info[f] = I;
    }
}

}  // namespace pdt
