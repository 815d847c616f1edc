// pdt_tip_dcs.h -- decommutation of TIP minor frames: the DCS-2 platform messages they relay.  The satellite receives the
// ARGOS platforms on 401.65 MHz and relays each message -- platform ID, sensor data, its own time code, the measured Doppler word --
// inside the TIP stream (standalone_matlab/Functionized/POES.m:868-1311).  The rule is fixed here, once, for the kernels
// (pdt_tip_dcs.hip) and their host restatement (pdt_host_tip_dcs) alike:
//   input     pdt_frame records from any source, repaired or not.  A record is ELIGIBLE <=> complete == 1 and nbytes == 104; `inverted`
//             plays no part (records are upright already)
//   SLOTS     the DCS bytes of a frame are bytes[b] for the 32 values b of TIP_DCS_SLOT (POES.m:869-932, 0-based here); the time of slot
//             byte b is time + b * (0.1 / 104) (POES.m:257)
//   SEGMENTS  record i+1 continues record i <=> both are eligible and bit_index[i+1] - bit_index[i] == 832.  A segment is a maximal run
//             of such records, its stream S the concatenation of their slots.  An ineligible record belongs to no segment (skipped);
//             nothing is joined across a gap (the reference concatenates whatever frames it has)
//   HEAD      position k of a segment is a head <=> k + 2 lies inside the segment, S[k] == 0xD6, S[k+1] < channel_max (cfg; 0 means 8,
//             the reference uses 9 for NOAA-19, POES.m:942-946; 1 .. 16) and the high nibble c of S[k+2] is a valid length code: with
//             n1 = c >> 1, (c & 1) == ((n1 >> 2) ^ (n1 >> 1) ^ n1) & 1 -- the codes 0 3 5 6 9 A C F of POES.m:1195-1214.  Then
//             blocks = n1 + 1 and L = 12 + 4 blocks.  A D6 with a good channel byte and an invalid code is counted (bad_code) and is no
//             head (the reference takes 44 bytes).  A D6 that is the stream's first byte is a head like any other (the reference never
//             sees it)
//   ACCEPTED  within a segment, in ascending order, a head is accepted <=> k >= the end k' + L' of the previously accepted one; any other
//             head is SHADOWED and counted (the reference cuts a packet wherever a data byte pair looks like a head)
//   PACKET    of an accepted head: nbytes = min(L, segment_len - k), complete = (nbytes == L), bytes[0 .. nbytes) from the stream, the
//             rest zero; channel = S[k+1]; time_code = (S[k+3] & 31) << 16 | S[k+4] << 8 | S[k+5] (nbytes >= 6, else 0); id = big-endian
//             S[k+6 .. k+9] (nbytes >= 10, else 0; the reference's TXID, POES.m:1184); complete: w = the last three bytes, big-endian,
//             doppler_ok = (w has an even number of ones), doppler_raw = (int32)(w >> 1) - (1 << 22) (the reference prints
//             doppler_raw / 32.0, POES.m:1261-1271), both 0 otherwise; frame, slot = the record and the slot 0 .. 31 that hold the D6;
//             stream_index = the byte's position when every eligible record's slots are counted in record order; time = the time of
//             the D6 byte ITSELF (the reference stamps a packet with the time of the byte in front of its D6)
//   SUMMARY   records used, records skipped, segments, stream bytes, heads, shadowed, bad_code, packets, complete, doppler_bad
// Packets come out in ascending record order.
#pragma once
#include <stdint.h>
#include <string.h>

#ifndef __host__
#define __host__
#define __device__
#endif

namespace pdt {

constexpr int TIP_DCS_SLOTS = 32, TIP_DCS_MAXLEN = 44, TIP_DCS_FRAME_BITS = 832;
constexpr int TIP_DCS_TILE = 2048;                        // stream bytes of one tile = 64 records (pdt_tip_dcs_tile)
constexpr int TIP_DCS_TILE_RECS = TIP_DCS_TILE / TIP_DCS_SLOTS;

struct TipDcsRec {                 // (= pdt_frame of include/pdt.h)
    double time;
    int64_t bit_index, time_src;
    uint8_t inverted, nbytes, complete, pad;
    uint8_t bytes[104];
};

struct TipDcsChainRec {            // (= FrameRec, what the chain's frame kernels leave on the device: no time stamp, those live on the host)
    long long bit_index, time_src;
    unsigned char inverted, nbytes, complete, pad;
    unsigned char bytes[104];
};

struct TipDcsPacket {              // (= pdt_dcs_packet)
    double time;
    int64_t stream_index;
    uint32_t frame, time_code, id;
    int32_t doppler_raw;
    uint8_t slot, channel, blocks, nbytes, complete, doppler_ok, pad[2];
    uint8_t bytes[TIP_DCS_MAXLEN];
};

struct TipDcsSummary {             // (= pdt_dcs_summary)
    uint64_t used, skipped, segments, stream_bytes, heads, shadowed, bad_code, packets, complete, doppler_bad;
};

// the frame byte of slot s (written out: a table in memory would be two copies, the host's and the device's)
__host__ __device__ inline int tip_dcs_slot_byte(int s)
{
    constexpr uint8_t T[TIP_DCS_SLOTS] = { 18, 19, 24, 25, 28, 29, 32, 33, 40, 41, 44, 45, 52, 53, 56, 57,
                                           60, 61, 64, 65, 68, 69, 72, 73, 76, 77, 86, 87, 90, 91, 94, 95 };
    return T[s];
}

__host__ __device__ inline bool tip_dcs_eligible(uint8_t complete, uint8_t nbytes) { return complete == 1 && nbytes == 104; }

// cfg.channel_max -> the bound of the channel byte, or 0 for a value that is not allowed
__host__ __device__ inline unsigned tip_dcs_channel_max(uint32_t cfg) { return cfg == 0 ? 8u : cfg <= 16 ? cfg : 0u; }

__host__ __device__ inline bool tip_dcs_code_valid(unsigned c)
{
    const unsigned n1 = c >> 1;
    return (c & 1u) == (((n1 >> 2) ^ (n1 >> 1) ^ n1) & 1u);
}
__host__ __device__ inline int tip_dcs_blocks(unsigned c) { return (int)(c >> 1) + 1; }
__host__ __device__ inline int tip_dcs_len(unsigned c) { return 12 + 4 * tip_dcs_blocks(c); }

// what three bytes at a position with at least three bytes left say: 1 head, 2 bad code, 0 neither
__host__ __device__ inline int tip_dcs_classify(unsigned b0, unsigned b1, unsigned b2, unsigned channel_max)
{
    if (b0 != 0xD6u || b1 >= channel_max) return 0;
    return tip_dcs_code_valid(b2 >> 4) ? 1 : 2;
}

// the time of frame byte b of a frame stamped t: ONE expression for host and device, a multiplication and an addition (no contraction)
__host__ __device__ inline double tip_dcs_time(double t, int b) { return t + (double)b * (0.1 / 104); }

// the Doppler word of a complete packet of L bytes, and its parity
__host__ __device__ inline uint32_t tip_dcs_doppler_word(const uint8_t *s, int L) { return ((uint32_t)s[L - 3] << 16) | ((uint32_t)s[L - 2] << 8) | s[L - 1]; }
__host__ __device__ inline bool tip_dcs_even(uint32_t w) { return !(__builtin_popcount(w) & 1); }

// the packet whose D6 is s[0]; `left` = the bytes from there to the segment's end (>= 3)
__host__ __device__ inline void tip_dcs_packet(TipDcsPacket *P, const uint8_t *s, long long left, double frame_time, uint32_t frame, int slot,
                                               int64_t stream_index)
{
    const unsigned c = s[2] >> 4;
    const int L = tip_dcs_len(c), nb = left < L ? (int)left : L;
    memset(P, 0, sizeof *P);                                 // (the four bytes that pad the record included)
    P->time =tip_dcs_time(frame_time, tip_dcs_slot_byte(slot));
    P->stream_index = stream_index;
    P->frame = frame;
    P->time_code = nb >= 6 ? ((uint32_t)(s[3] & 31u) << 16) | ((uint32_t)s[4] << 8) | s[5] : 0u;
    P->id = nb >= 10 ? ((uint32_t)s[6] << 24) | ((uint32_t)s[7] << 16) | ((uint32_t)s[8] << 8) | s[9] : 0u;
    P->slot = (uint8_t)slot;
    P->channel = s[1];
    P->blocks = (uint8_t)tip_dcs_blocks(c);
    P->nbytes = (uint8_t)nb;
    P->complete = nb == L;
    P->pad[0] = P->pad[1] = 0;
    for (int k = 0; k < TIP_DCS_MAXLEN; k++) P->bytes[k] = k < nb ? s[k] : 0;
    if (nb == L) {
        const uint32_t w = tip_dcs_doppler_word(s, L);
        P->doppler_ok = tip_dcs_even(w);
        P->doppler_raw = (int32_t)(w >> 1) - (1 << 22);
    } else {
        P->doppler_ok = 0;
        P->doppler_raw = 0;
    }
}

// The rule on the host, straight from its text.  At most cap packets are written; the count and the summary are always complete.
// S: scratch of 32 n bytes (the caller's, so that this header allocates nothing)
inline uint64_t tip_dcs_host(const TipDcsRec *recs, uint64_t n, unsigned channel_max, uint8_t *S, TipDcsPacket *out, uint64_t cap, TipDcsSummary *sum)
{
    memset(sum, 0, sizeof *sum);
    uint64_t i = 0, eligible_before = 0;
    while (i < n) {
        if (!tip_dcs_eligible(recs[i].complete, recs[i].nbytes)) {
            sum->skipped++;
            i++;
            continue;
        }
        uint64_t j = i + 1;
        while (j < n && tip_dcs_eligible(recs[j].complete, recs[j].nbytes) && recs[j].bit_index - recs[j - 1].bit_index == TIP_DCS_FRAME_BITS) j++;
        const long long len = (long long)(j - i) * TIP_DCS_SLOTS;
        for (uint64_t r = i; r < j; r++)
            for (int s = 0; s < TIP_DCS_SLOTS; s++) S[(r - i) * TIP_DCS_SLOTS + s] = recs[r].bytes[tip_dcs_slot_byte(s)];
        sum->segments++;
        sum->used += j - i;
        sum->stream_bytes += (uint64_t)len;
        long long end = 0;
        for (long long k = 0; k + 2 < len; k++) {
            const int what = tip_dcs_classify(S[k], S[k + 1], S[k + 2], channel_max);
            if (what == 2) sum->bad_code++;
            if (what != 1) continue;
            sum->heads++;
            if (k < end) {
                sum->shadowed++;
                continue;
            }
            end = k + tip_dcs_len(S[k + 2] >> 4);
            TipDcsPacket P;
            const uint64_t r = i + (uint64_t)(k / TIP_DCS_SLOTS);
            tip_dcs_packet(&P, S + k, len - k, recs[r].time, (uint32_t)r, (int)(k % TIP_DCS_SLOTS), (int64_t)(eligible_before * TIP_DCS_SLOTS) + k);
            if (sum->packets < cap) memcpy(out + sum->packets, &P, sizeof P);
            sum->packets++;
            sum->complete += P.complete;
            sum->doppler_bad += P.complete && !P.doppler_ok;
        }
        eligible_before += j - i;
        i = j;
    }
    return sum->packets;
}

}  // namespace pdt
