// pdt_tip_subcom.h -- decommutation of TIP minor frames: subcommutated bytes.  A fixed byte of the minor frame belongs to
// a different measurement depending on the frame's 9-bit minor-frame counter.  SEM-2, the space environment monitor, reads out its 22
// MEPED and 38 TED channels this way through bytes 20 and 21 (standalone_matlab/Functionized/POES.m:1314-1700), the 16-second analogue
// housekeeping points use bytes 11 and 14 (POES.m:462-513), SBUV others.  One table-driven rule covers them all; it is fixed here, once,
// for the kernels (pdt_tip_subcom.hip) and their host restatement (pdt_host_tip_subcom) alike:
//   input     pdt_frame records from any source, repaired or not.  A record is ELIGIBLE <=> complete == 1 and nbytes == 104 (tip_dcs_eligible).
//             Its counter is id = (bytes[4] & 1) << 8 | bytes[5].  An eligible record with id >= 320 is counted bad_id and yields nothing;
//             an ineligible record is counted skipped; every other record is USED
//   TABLE     1 .. 256 entries {channel, byte, period, phase, mask, shift, invert}: channel < 128, byte 0 .. 103, period divides 320,
//             phase < period, mask != 0, shift 0 .. 7, invert 0 or 1; anything else is an argument error.  Entries need not be sorted;
//             nchan = the largest channel + 1, empty channels are allowed
//   FIRES     an entry fires in a used record <=> id % period == phase.  raw = bytes[byte], value = ((invert ? 255 - raw : raw) & mask) >> shift
//   SAMPLE    every firing is a sample: time = tip_dcs_time(record's time, byte), frame = the record's index, minor_id = id, channel,
//             entry = the entry's index, value, raw, and flags:
//               BYTE_PARITY (1)  the even-parity group that covers `byte` fails: group g = 0 .. 4 covers bytes 2 + 17 g .. 18 + 17 g against
//                                bit 5 - g of bytes[103] (pdt_tip_repair.h's groups, through its functions)
//               ID_PARITY   (2)  group 0 fails: it covers bytes 4 and 5, so the counter that chose the channel is in doubt
//               UNCOVERED   (4)  `byte` lies in no group (0, 1, 87 .. 103)
//               SPIKE       (8)  see below
//             With trusted_only a sample with bit 1 or bit 2 set is counted `dropped` and does not exist for anything that follows: not
//             for the order, the spike test, the counts samples, byte_parity and id_parity (both 0 then), channels_hit
//   ORDER     channel-major: channel 0's samples, then channel 1's ...; within a channel ascending by (record, entry index).
//             offsets[0 .. nchan] gives each channel's place and is always complete, whatever cap is
//   SPIKE     sample j of a channel is a spike <=> both neighbours j - 1 and j + 1 lie in the same channel and |v[j-1] - v[j]| > thr and
//             |v[j+1] - v[j]| > thr, on the values as decoded; thr = spike_threshold, 0 means 20 (the reference's FilterThreshold), above
//             255 is an argument error
//   SUMMARY   used, skipped, bad_id, samples, dropped, byte_parity, id_parity, spikes, channels_hit (channels with a sample)
// Three departures from POES.m:1379-1490:
//   - the reference zeroes a spike in place, so its test of the next sample sees the zero: a sequential dependence, and a lost value.
//     Here a spike is flagged and keeps its value, and every test sees the values as decoded
//   - the reference's series start with a dummy 0 (X(1) = 0).  Here a channel's first and last sample never spike
//   - neighbours are neighbours in the series whatever gap lies between them (as in the reference)
#pragma once
#include <stdint.h>
#include <string.h>

#include "pdt_tip_dcs.h"
#include "pdt_tip_repair.h"

namespace pdt {

constexpr int TIP_SUBCOM_MAX_ENTRIES = 256, TIP_SUBCOM_MAX_CHANNELS = 128, TIP_SUBCOM_CYCLE = 320, TIP_SUBCOM_FRAME_BYTES = 104;
constexpr int TIP_SUBCOM_TILE = 64;                        // records of one tile = one wavefront (pdt_tip_subcom_tile)
constexpr unsigned TIP_SUBCOM_BYTE_PARITY = 1, TIP_SUBCOM_ID_PARITY = 2, TIP_SUBCOM_UNCOVERED = 4, TIP_SUBCOM_SPIKE = 8;
constexpr int TIP_SUBCOM_SEM = 0, TIP_SUBCOM_HK = 1;       // the built-in tables
constexpr int TIP_SUBCOM_SEM_ENTRIES = 76, TIP_SUBCOM_SEM_CHANNELS = 60, TIP_SUBCOM_HK_ENTRIES = 5, TIP_SUBCOM_HK_CHANNELS = 5;

struct TipSubcomEntry {            // (= pdt_subcom_entry)
    uint8_t channel, byte;
    uint16_t period, phase;
    uint8_t mask, shift, invert, pad;
};

struct TipSubcomSample {           // (= pdt_subcom_sample)
    double time;
    uint32_t frame;
    uint16_t minor_id;
    uint8_t channel, entry, value, raw, flags, pad[5];
};

struct TipSubcomSummary {          // (= pdt_subcom_summary)
    uint64_t used, skipped, bad_id, samples, dropped, byte_parity, id_parity, spikes, channels_hit;
};

__host__ __device__ inline bool tip_subcom_entry_valid(const TipSubcomEntry &e)
{
    return e.channel < TIP_SUBCOM_MAX_CHANNELS && e.byte < TIP_SUBCOM_FRAME_BYTES && e.period != 0 && TIP_SUBCOM_CYCLE % e.period == 0 && e.phase < e.period &&
           e.mask != 0 && e.shift <= 7 && e.invert <= 1;
}

// a table -> nchan, or 0 for one that is not allowed
inline int tip_subcom_table_channels(const TipSubcomEntry *tab, uint64_t ne)
{
    if (!tab || ne < 1 || ne > (uint64_t)TIP_SUBCOM_MAX_ENTRIES) return 0;
    int nchan = 0;
    for (uint64_t e = 0; e < ne; e++) {
        if (!tip_subcom_entry_valid(tab[e])) return 0;
        if (tab[e].channel + 1 > nchan) nchan = tab[e].channel + 1;
    }
    return nchan;
}

// the most entries that fire in one record: records * this bounds the samples
inline int tip_subcom_table_max_fire(const TipSubcomEntry *tab, int ne)
{
    int most = 0;
    for (int id = 0; id < TIP_SUBCOM_CYCLE; id++) {
        int f = 0;
        for (int e = 0; e < ne; e++) f += id % tab[e].period == tab[e].phase;
        if (f > most) most = f;
    }
    return most;
}

// cfg.spike_threshold -> thr, or -1 for a value that is not allowed
__host__ __device__ inline int tip_subcom_threshold(uint32_t cfg) { return cfg == 0 ? 20 : cfg <= 255 ? (int)cfg : -1; }

__host__ __device__ inline unsigned tip_subcom_id(const uint8_t *bytes) { return ((unsigned)(bytes[4] & 1u) << 8) | bytes[5]; }

// the parity group that covers a frame byte, or -1: the byte's first frame bit against pdt_tip_repair.h's constants
__host__ __device__ inline int tip_subcom_group(int byte)
{
    const int j = 8 * byte - TIP_REPAIR_FIRST;
    return j >= 0 && j < TIP_REPAIR_GROUPS * TIP_REPAIR_DATA ? j / TIP_REPAIR_DATA : -1;
}

// bit g set <=> group g of the record fails
__host__ __device__ inline unsigned tip_subcom_failed(const uint8_t *bytes)
{
    unsigned failed = 0;
    for (int g = 0; g < TIP_REPAIR_GROUPS; g++) {
        unsigned odd = tip_repair_parity_bit(bytes, g);
        for (int t = 0; t < TIP_REPAIR_DATA / 8; t++) odd ^= tip_repair_byte_odd(bytes, g, t);
        failed |= odd << g;
    }
    return failed;
}

// What the rule needs of a record, in one word: the counter (bits 0 .. 8), the failing groups (9 .. 13), used (14), bad_id (15)
constexpr unsigned TIP_SUBCOM_M_USED = 1u << 14, TIP_SUBCOM_M_BAD_ID = 1u << 15;
__host__ __device__ inline unsigned tip_subcom_mark(uint8_t complete, uint8_t nbytes, const uint8_t *bytes)
{
    if (!tip_dcs_eligible(complete, nbytes)) return 0u;
    const unsigned id = tip_subcom_id(bytes);
    return id | (tip_subcom_failed(bytes) << 9) | (id < (unsigned)TIP_SUBCOM_CYCLE ? TIP_SUBCOM_M_USED : TIP_SUBCOM_M_BAD_ID);
}
__host__ __device__ inline unsigned tip_subcom_mark_id(unsigned m) { return m & 511u; }
__host__ __device__ inline unsigned tip_subcom_mark_failed(unsigned m) { return (m >> 9) & 31u; }

__host__ __device__ inline bool tip_subcom_fires(const TipSubcomEntry &e, unsigned id) { return id % e.period == e.phase; }

__host__ __device__ inline unsigned tip_subcom_value(const TipSubcomEntry &e, unsigned raw) { return ((e.invert ? 255u - raw : raw) & e.mask) >> e.shift; }

// the flags of a sample of frame byte `byte` in a record whose failing groups are `failed` (without SPIKE)
__host__ __device__ inline unsigned tip_subcom_flags(int byte, unsigned failed)
{
    const int g = tip_subcom_group(byte);
    return (g >= 0 && ((failed >> g) & 1u) ? TIP_SUBCOM_BYTE_PARITY : 0u) | (failed & 1u ? TIP_SUBCOM_ID_PARITY : 0u) | (g < 0 ? TIP_SUBCOM_UNCOVERED : 0u);
}
__host__ __device__ inline bool tip_subcom_untrusted(unsigned flags) { return (flags & (TIP_SUBCOM_BYTE_PARITY | TIP_SUBCOM_ID_PARITY)) != 0; }

__host__ __device__ inline bool tip_subcom_is_spike(int before, int v, int after, int thr)
{
    const int a = before > v ? before - v : v - before, b = after > v ? after - v : v - after;
    return a > thr && b > thr;
}

__host__ __device__ inline TipSubcomSample tip_subcom_sample(double frame_time, uint32_t frame, unsigned id, const TipSubcomEntry &e, int entry, unsigned raw,
                                                             unsigned flags)
{
    TipSubcomSample s;
    s.time = tip_dcs_time(frame_time, e.byte);
    s.frame = frame;
    s.minor_id = (uint16_t)id;
    s.channel = e.channel;
    s.entry = (uint8_t)entry;
    s.value = (uint8_t)tip_subcom_value(e, raw);
    s.raw = (uint8_t)raw;
    s.flags = (uint8_t)flags;
    for (int k = 0; k < 5; k++) s.pad[k] = 0;
    return s;
}

// The rule on the host, straight from its text, in two steps so that this header allocates nothing.  Step 1: everything of the summary
// but the spikes, and offsets[0 .. nchan].
inline void tip_subcom_host_count(const TipDcsRec *recs, uint64_t n, const TipSubcomEntry *tab, int ne, int nchan, bool trusted_only, uint64_t *offsets,
                                  TipSubcomSummary *sum)
{
    memset(sum, 0, sizeof *sum);
    for (int c = 0; c <= nchan; c++) offsets[c] = 0;
    for (uint64_t i = 0; i < n; i++) {
        const unsigned m = tip_subcom_mark(recs[i].complete, recs[i].nbytes, recs[i].bytes);
        if (!(m & TIP_SUBCOM_M_USED)) {
            if (m & TIP_SUBCOM_M_BAD_ID) sum->bad_id++;
            else sum->skipped++;
            continue;
        }
        sum->used++;
        for (int e = 0; e < ne; e++) {
            if (!tip_subcom_fires(tab[e], tip_subcom_mark_id(m))) continue;
            const unsigned fl = tip_subcom_flags(tab[e].byte, tip_subcom_mark_failed(m));
            if (trusted_only && tip_subcom_untrusted(fl)) {
                sum->dropped++;
                continue;
            }
            sum->samples++;
            sum->byte_parity += (fl & TIP_SUBCOM_BYTE_PARITY) != 0;
            sum->id_parity += (fl & TIP_SUBCOM_ID_PARITY) != 0;
            offsets[tab[e].channel + 1]++;
        }
    }
    for (int c = 0; c < nchan; c++) {
        sum->channels_hit += offsets[c + 1] != 0;
        offsets[c + 1] += offsets[c];
    }
}

// Step 2: the samples in their order -- at most cap are written -- and the spikes.  cursor: scratch of nchan words; V: scratch of
// offsets[nchan] bytes, every sample's value at its place
inline void tip_subcom_host_fill(const TipDcsRec *recs, uint64_t n, const TipSubcomEntry *tab, int ne, int nchan, bool trusted_only, int thr, const uint64_t *offsets,
                                 uint64_t *cursor, uint8_t *V, TipSubcomSample *out, uint64_t cap, TipSubcomSummary *sum)
{
    for (int c = 0; c < nchan; c++) cursor[c] = offsets[c];
    for (uint64_t i = 0; i < n; i++) {
        const unsigned m = tip_subcom_mark(recs[i].complete, recs[i].nbytes, recs[i].bytes);
        if (!(m & TIP_SUBCOM_M_USED)) continue;
        for (int e = 0; e < ne; e++) {
            if (!tip_subcom_fires(tab[e], tip_subcom_mark_id(m))) continue;
            const unsigned fl = tip_subcom_flags(tab[e].byte, tip_subcom_mark_failed(m));
            if (trusted_only && tip_subcom_untrusted(fl)) continue;
            const TipSubcomSample s = tip_subcom_sample(recs[i].time, (uint32_t)i, tip_subcom_mark_id(m), tab[e], e, recs[i].bytes[tab[e].byte], fl);
            const uint64_t at = cursor[tab[e].channel]++;
            V[at] = s.value;
            if (at < cap) memcpy(out + at, &s, sizeof s);
        }
    }
    for (int c = 0; c < nchan; c++)
        for (uint64_t j = offsets[c] + 1; j + 1 < offsets[c + 1]; j++)
            if (tip_subcom_is_spike(V[j - 1], V[j], V[j + 1], thr)) {
                sum->spikes++;
                if (j < cap) out[j].flags |= (uint8_t)TIP_SUBCOM_SPIKE;
            }
}

// The built-in tables (POES.m:1340-1377, 1561-1621, 462-513).  SEM: a = byte 20, b = byte 21, sent complemented (POES.m:1317-1318)
inline void tip_subcom_put(TipSubcomEntry *t, int *n, int channel, int byte, int period, int phase, int invert, int mask = 0xFF, int shift = 0)
{
    t[(*n)++] = TipSubcomEntry{ (uint8_t)channel, (uint8_t)byte, (uint16_t)period, (uint16_t)phase, (uint8_t)mask, (uint8_t)shift, (uint8_t)invert, 0 };
}

// which -> the entries (t holds TIP_SUBCOM_MAX_ENTRIES); returns their number, 0 for a table that does not exist
inline int tip_subcom_builtin(int which, TipSubcomEntry *t)
{
    int n = 0;
    if (which == TIP_SUBCOM_HK) {
        tip_subcom_put(t, &n, 0, 11, 80, 48, 0);           // STX1 (POES.m:492-500)
        tip_subcom_put(t, &n, 1, 11, 80, 50, 0);           // STX2
        tip_subcom_put(t, &n, 2, 11, 80, 40, 0);           // STX3
        tip_subcom_put(t, &n, 3, 14, 160, 114, 0);         // SARR-A (POES.m:503-508; line 506 names the wrong array, the counter is the same)
        tip_subcom_put(t, &n, 4, 14, 160, 2, 0);           // SARR-B
        return n;
    }
    if (which != TIP_SUBCOM_SEM) return 0;
    const int a = 20, b = 21;
    // MEPED: channels 0 .. 21
    tip_subcom_put(t, &n, 0, b, 20, 0, 1);
    for (int p = 1; p <= 9; p++) {
        tip_subcom_put(t, &n, 2 * p - 1, a, 20, p, 1);
        tip_subcom_put(t, &n, 2 * p, b, 20, p, 1);
    }
    tip_subcom_put(t, &n, 19, a, 20, 10, 1);
    tip_subcom_put(t, &n, 20, b, 40, 10, 1);
    tip_subcom_put(t, &n, 21, b, 40, 30, 1);
    // TED, every 20 frames: channels 22 .. 37
    for (int k = 0; k < 4; k++) {
        tip_subcom_put(t, &n, 22 + 2 * k, a, 20, 13 + k, 1);
        tip_subcom_put(t, &n, 23 + 2 * k, b, 20, 13 + k, 1);
    }
    tip_subcom_put(t, &n, 30, a, 20, 17, 1, 0xF0, 4);
    tip_subcom_put(t, &n, 31, a, 20, 17, 1, 0x0F, 0);
    tip_subcom_put(t, &n, 32, b, 20, 17, 1);
    tip_subcom_put(t, &n, 33, a, 20, 18, 1);
    tip_subcom_put(t, &n, 34, b, 20, 18, 1, 0xF0, 4);
    tip_subcom_put(t, &n, 35, b, 20, 18, 1, 0x0F, 0);
    tip_subcom_put(t, &n, 36, a, 20, 19, 1);
    tip_subcom_put(t, &n, 37, b, 20, 19, 1);
    // TED, the counters that end in 1 (channels 38 .. 48) and those that end in 2 (49 .. 59)
    for (int h = 0; h < 2; h++) {
        const int c = h ? 49 : 38, s = c + 4;
        tip_subcom_put(t, &n, c, a, 80, 11 + h, 1);
        tip_subcom_put(t, &n, c + 1, b, 80, 11 + h, 1);
        tip_subcom_put(t, &n, c + 2, a, 80, 31 + h, 1);
        tip_subcom_put(t, &n, c + 3, b, 80, 31 + h, 1);
        for (int id = 51; id <= 211; id += 80) {
            tip_subcom_put(t, &n, s, a, 320, id + h, 1);
            tip_subcom_put(t, &n, s + 1, b, 320, id + h, 1);
        }
        for (int id = 71; id <= 231; id += 80) {
            tip_subcom_put(t, &n, s + 2, a, 320, id + h, 1);
            tip_subcom_put(t, &n, s + 3, b, 320, id + h, 1);
        }
        tip_subcom_put(t, &n, s + 4, a, 320, 291 + h, 1);
        tip_subcom_put(t, &n, s + 5, b, 320, 291 + h, 1);
        tip_subcom_put(t, &n, s + 6, b, 320, 311 + h, 1);  // (the reference ignores a there; so does the table)
    }
    return n;
}

inline const char *tip_subcom_builtin_name(int which, int channel)
{
    static const char *const sem[TIP_SUBCOM_SEM_CHANNELS] = {
        "0P1", "0P2", "0P3", "0P4", "0P5", "0P6", "0E1", "0E2", "0E3", "9P1", "9P2", "9P3", "9P4", "9P5", "9P6", "9E1", "9E2", "9E3", "P6", "P7", "P8", "P9",
        "0EFL", "3EFL", "0PFL", "3PFL", "0EFH", "3EFH", "0PFH", "3PFH", "0EM", "0PM", "0DEM", "0DPM", "3EM", "3PM", "3DEM", "3DPM",
        "0DE1", "0DE2", "3DE1", "3DE2", "0DP1", "0DP2", "3DP1", "3DP2", "0EBKL", "0EBKH", "3PBKL",
        "0DE3", "0DE4", "3DE3", "3DE4", "0DP3", "0DP4", "3DP3", "3DP4", "0PBKL", "0PBKH", "3PBKH" };
    static const char *const hk[TIP_SUBCOM_HK_CHANNELS] = { "STX1", "STX2", "STX3", "SARR-A", "SARR-B" };
    if (channel < 0) return nullptr;
    if (which == TIP_SUBCOM_SEM) return channel < TIP_SUBCOM_SEM_CHANNELS ? sem[channel] : nullptr;
    if (which == TIP_SUBCOM_HK) return channel < TIP_SUBCOM_HK_CHANNELS ? hk[channel] : nullptr;
    return nullptr;
}

}  // namespace pdt
