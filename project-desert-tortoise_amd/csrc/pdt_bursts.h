// pdt_bursts.h -- short transmissions in a wideband capture: the spectrum over time (waterfall) of a stretch and the bursts in it
// (DESIGN 4.13).  It stands on the survey's pieces (pdt_survey.h) unchanged; what is new is fixed here, once, for the kernels
// (pdt_bursts.hip) and their host restatement (pdt_host_bursts) alike:
//   segment s = the survey's: ddc_load<FMT>, Blackman window, radix-4 DIF passes, survey_power; N in {1024, 4096, 16384}
//   row t     = segments t R .. t R + R - 1 of the stretch, 1 <= R <= BURST_MAX_ROWS_PER; a last incomplete row is dropped
//   W[t][b]   = the row's R segment powers of bin b added in float in ascending order from 0 -- no division
//   floor     = survey_floor of the survey's averaged spectrum P of the same stretch at the same N (all whole segments of the
//               stretch, those of a dropped last row included: P is the survey's, as it is)
//   level     = (float)(floor 10^(threshold_db / 10) R), the product in double in this order (burst_level)
//   peaks of a row: a bin's key = the bits of W when W > 0, else 0 (so NaN, zero and blanked bins are never taken, and keys order
//               as the powers do); repeatedly the bin of the largest key, of equal keys the lowest bin; stop when the key is 0, when
//               W < level (in float), or at BURST_ROW_PEAKS peaks; the record is (bin, W[b - 1], W[b], W[b + 1]) of the row as it was
//               before any blanking, the neighbours wrapping at the band's edge; then the keys of the bins within
//               gb = min(floor(guard_hz / binw), N / 2) of b become 0 (burst_row_peaks; the kernel does the same in parallel)
//   linking   (burst_link, host only): rows in ascending order, a row's peaks in the order found.  A peak continues the open track,
//               not yet continued in this row, whose last bin is nearest (circular distance), at most mb = min(floor(merge_hz /
//               binw), N / 2 - 1) bins away; of equally near ones the track with the lower last bin; else it opens a track.  A track
//               whose last peak lies more than gap_rows + 1 rows back closes before the row's peaks are looked at; at the end all close.
//               A closed track of rows = last_row - first_row + 1 (rows without a peak in between count) is a burst when
//               duration_s = (rows R N) / Fs_in >= min_s and (max_s == 0 or duration_s <= max_s)
//   a burst's offset: every peak of the track, in row order, gives c = (sum over k in {-1, 0, 1} of k u_k) / (sum of u_k),
//               u_k = max(W[b + k] - floor R, 0) in double (0 when the sum is 0), and the place d + c, d = the track's first bin as a
//               signed bin (b < N / 2 ? b : b - N) plus the peak's circular distance from it; offset_hz = (sum of W[b] (d + c)) /
//               (sum of W[b]) binw, wrapped into [-Fs_in / 2, Fs_in / 2)
//   peak_db   = (float)(10 log10(the track's largest W[b] / (floor R))); floor_power = (float)floor
//   bursts come back ordered by first_row, then offset_hz
//   sidebands (burst_link): a transmitter's modulation does not end at guard_hz -- the envelope of a biphase signal of half-bit T
//               falls as 1 / (pi f T)^2, for ARGOS (T = 1 / 800 s) 36 dB down at 16 kHz, 48 dB at 64 kHz, and a platform 55 dB over the
//               floor still stands 19 dB over it just outside the guard.  A peak is therefore not linked when THE SAME ROW holds a
//               peak at most BURST_SIDEBAND_GUARDS gb bins away (circular) whose power is at least 10^(BURST_SIDEBAND_DB / 10) times
//               its own (the product in double): evidence of one row, bounded in frequency.  Farther away, or against anything
//               less than 25 dB stronger, every peak counts; the rows' peak records themselves are not touched
//   platforms (burst_carriers): the bursts sorted by offset_hz (then by their order); neighbours in that order at most merge_hz apart
//               belong to one platform; its offset = the mean of its bursts' offsets weighted by 10^(peak_db / 10), in that order, in
//               double; its peak_db and floor_power those of its strongest burst (the first of equals); strongest platform first,
//               of equal ones the lower offset
#pragma once
#include <math.h>
#include <stdint.h>
#include <string.h>
#include <algorithm>
#include <vector>
#include "pdt_survey.h"

namespace pdt {

constexpr int BURST_ROW_PEAKS = 8;              // peaks recorded per row
constexpr int BURST_MAX_ROWS_PER = SURVEY_RUN;  // R: at most the survey's run
constexpr int BURST_DEFAULT_ROWS_PER = 8;
constexpr int BURST_DEFAULT_NFFT = 4096;
constexpr int BURST_DEFAULT_GAP_ROWS = 1;
constexpr double BURST_SIDEBAND_DB = 25.0;      // a peak beside one this much stronger in its row, at most ...
constexpr int BURST_SIDEBAND_GUARDS = 4;        // ... this many guards away, is its sideband (burst_link)
constexpr int BURST_BATCH_SEGS = 64;            // segments one workgroup of the waterfall takes: max(1, 64 / R) consecutive rows
constexpr size_t BURST_SLAB_BYTES = (size_t)64 << 20;       // the rows resident at a time (the developer switch PDT_BURST_SLAB_ROWS: rows)

struct BurstPeak {                 // (= pdt_row_peak of include/pdt.h), 16 bytes
    int32_t bin;
    float below, power, above;     // W[bin - 1], W[bin], W[bin + 1]
};

struct BurstPlan {
    int nfft, rows_per, gap_rows;
    double threshold_db, guard_hz, merge_hz, min_s, max_s;
    uint64_t first, nrows;           // the stretch's first frame, its whole rows
};

struct Burst {                     // (= pdt_burst of include/pdt.h)
    uint64_t first_row, rows;
    double start_s, duration_s, offset_hz;
    float peak_db, floor_power;
};

__host__ __device__ __forceinline__ uint32_t burst_key(float w)
{
    uint32_t u;
    memcpy(&u, &w, 4);
    return w > 0.0f ? u : 0u;
}

inline float burst_level(double floor, double threshold_db, int rows_per)
{
    return (float)(floor * pow(10.0, threshold_db / 10.0) * (double)rows_per);
}

inline int burst_guard_bins(double guard_hz, double in_rate, int n)
{
    return (int)std::min<double>(std::floor(guard_hz / (in_rate / (double)n)), (double)(n / 2));
}

inline int burst_merge_bins(double merge_hz, double in_rate, int n)
{
    return (int)std::min<double>(std::floor(merge_hz / (in_rate / (double)n)), (double)(n / 2 - 1));
}

// the peaks of one row W (natural bin order); returns their number
inline int burst_row_peaks(const float *W, int n, float level, int gb, BurstPeak *out)
{
    std::vector<uint32_t> key((size_t)n);
    for (int i = 0; i < n; i++) key[(size_t)i] = burst_key(W[i]);
    int count = 0;
    while (count < BURST_ROW_PEAKS) {
        int b = 0;
        for (int i = 1; i < n; i++)
            if (key[(size_t)i] > key[(size_t)b]) b = i;
        if (!key[(size_t)b] || W[b] < level) break;
        out[count].bin = b;
        out[count].below = W[(b + n - 1) % n];
        out[count].power = W[b];
        out[count].above = W[(b + 1) % n];
        count++;
        for (int k = -gb; k <= gb; k++) key[(size_t)((b + k + n) % n)] = 0;
    }
    return count;
}

// b's circular distance from a, in (-n / 2, n / 2]
inline int burst_delta(int a, int b, int n)
{
    int d = (b - a) % n;
    if (d < 0) d += n;
    return d > n / 2 ? d - n : d;
}

// The bursts of the rows' peaks, ordered by start, then offset.  Row t's counts[t] peaks follow each other in peaks[]; the rows' peaks
// follow each other without gaps (compact), or row t's begin at t BURST_ROW_PEAKS.
inline std::vector<Burst> burst_link(const BurstPeak *peaks, const int *counts, bool compact, const BurstPlan &p, double floor, double in_rate)
{
    struct Track {
        uint64_t first_row, last_row;
        int first_bin, last_bin;
        double sw, swd, peak;
    };
    const int n = p.nfft, mb = burst_merge_bins(p.merge_hz, in_rate, n);
    const int sb = (int)std::min<long long>((long long)BURST_SIDEBAND_GUARDS * burst_guard_bins(p.guard_hz, in_rate, n), n / 2);
    const double binw = in_rate / (double)n, floor_r = floor * (double)p.rows_per, side = pow(10.0, BURST_SIDEBAND_DB / 10.0);
    size_t next = 0;
    std::vector<Track> open;
    std::vector<Burst> out;
    auto close = [&](const Track &k) {
        Burst b;
        b.first_row = k.first_row;
        b.rows = k.last_row - k.first_row + 1;
        b.start_s = ((double)p.first + (double)k.first_row * (double)p.rows_per * (double)n) / in_rate;
        b.duration_s = (double)b.rows * (double)p.rows_per * (double)n / in_rate;
        if (b.duration_s < p.min_s || (p.max_s != 0 && b.duration_s > p.max_s)) return;
        double f = (k.sw > 0.0 ? k.swd / k.sw : (double)(k.first_bin < n / 2 ? k.first_bin : k.first_bin - n)) * binw;
        if (f >= 0.5 * in_rate) f -= in_rate;
        if (f < -0.5 * in_rate) f += in_rate;
        b.offset_hz = f;
        b.peak_db = (float)(10.0 * log10(k.peak / floor_r));
        b.floor_power = (float)floor;
        out.push_back(b);
    };
    std::vector<unsigned char> taken;
    for (uint64_t t = 0; t < p.nrows; t++) {
        size_t keep = 0;
        for (size_t i = 0; i < open.size(); i++) {
            if (t - open[i].last_row > (uint64_t)p.gap_rows + 1) close(open[i]);
            else open[keep++] = open[i];
        }
        open.resize(keep);
        taken.assign(open.size(), 0);
        const BurstPeak *row = peaks + (compact ? next : (size_t)t * BURST_ROW_PEAKS);
        next += (size_t)counts[t];
        for (int k = 0; k < counts[t]; k++) {
            const BurstPeak &pk = row[k];
            bool sideband = false;
            for (int j = 0; j < counts[t] && !sideband; j++)
                sideband = j != k && std::abs(burst_delta(row[j].bin, pk.bin, n)) <= sb && (double)row[j].power >= (double)pk.power * side;
            if (sideband) continue;
            int best = -1, best_d = 0;
            for (size_t i = 0; i < taken.size(); i++) {             // (tracks opened in this row are beyond taken.size())
                if (taken[i]) continue;
                const int d = std::abs(burst_delta(open[i].last_bin, pk.bin, n));
                if (d > mb) continue;
                if (best < 0 || d < best_d || (d == best_d && open[i].last_bin < open[(size_t)best].last_bin)) {
                    best = (int)i;
                    best_d = d;
                }
            }
            if (best < 0) {
                Track k0 = { t, t, pk.bin, pk.bin, 0.0, 0.0, 0.0 };
                open.push_back(k0);
                best = (int)open.size() - 1;
            } else {
                taken[(size_t)best] = 1;
            }
            Track &tr = open[(size_t)best];
            const double u0 = std::max((double)pk.below - floor_r, 0.0), u1 = std::max((double)pk.power - floor_r, 0.0),
                         u2 = std::max((double)pk.above - floor_r, 0.0), su = u0 + u1 + u2;
            const double c = su > 0.0 ? (u2 - u0) / su : 0.0;
            const double d = (double)(tr.first_bin < n / 2 ? tr.first_bin : tr.first_bin - n) + (double)burst_delta(tr.first_bin, pk.bin, n);
            tr.sw = tr.sw + (double)pk.power;
            tr.swd = tr.swd + (double)pk.power * (d + c);
            tr.peak = std::max(tr.peak, (double)pk.power);
            tr.last_row = t;
            tr.last_bin = pk.bin;
        }
    }
    for (size_t i = 0; i < open.size(); i++) close(open[i]);
    std::stable_sort(out.begin(), out.end(), [](const Burst &a, const Burst &b) {
        return a.first_row != b.first_row ? a.first_row < b.first_row : a.offset_hz < b.offset_hz;
    });
    return out;
}

// the platforms of a burst list, strongest first
inline std::vector<SurveyCarrier> burst_carriers(const Burst *b, int count, double merge_hz)
{
    std::vector<int> idx((size_t)count);
    for (int i = 0; i < count; i++) idx[(size_t)i] = i;
    std::stable_sort(idx.begin(), idx.end(), [&](int x, int y) { return b[x].offset_hz < b[y].offset_hz; });
    std::vector<SurveyCarrier> out;
    for (int i = 0; i < count;) {
        int j = i + 1;
        while (j < count && b[idx[(size_t)j]].offset_hz - b[idx[(size_t)(j - 1)]].offset_hz <= merge_hz) j++;
        double sw = 0.0, swf = 0.0;
        int top = idx[(size_t)i];
        for (int k = i; k < j; k++) {
            const Burst &e = b[idx[(size_t)k]];
            const double w = pow(10.0, (double)e.peak_db / 10.0);
            sw = sw + w;
            swf = swf + w * e.offset_hz;
            if (e.peak_db > b[top].peak_db) top = idx[(size_t)k];
        }
        SurveyCarrier c;
        c.offset_hz = sw > 0.0 && std::isfinite(sw) ? swf / sw : b[top].offset_hz;
        c.peak_db = b[top].peak_db;
        c.floor_power = b[top].floor_power;
        out.push_back(c);
        i = j;
    }
    std::stable_sort(out.begin(), out.end(), [](const SurveyCarrier &x, const SurveyCarrier &y) {
        return x.peak_db != y.peak_db ? x.peak_db > y.peak_db : x.offset_hz < y.offset_hz;
    });
    return out;
}

}  // namespace pdt
