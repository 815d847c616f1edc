// pdt_ffp.hip -- feed-forward POES bits of a whole stream (pdt_ffp.h): the kernel that takes the measured carrier out segment by segment
// (k_ffp_mix), the exhaustive search of the bit clock block by block (k_ffp_search), the choice of every block's clock phase, its
// unwrapping and the blocks' bit ranges (k_ffp_track), the decisions (k_ffp_bits), their launch, and the host restatement
// pdt_host_ffp_bits / pdt_host_ffp_mix.  A unit of its own, beside pdt_ff.hip and pdt_tip_sync.hip.
#include <hip/hip_runtime.h>
#include <math.h>
#include <string.h>
#include <algorithm>
#include <vector>

#include "../../include/pdt.h"
#include "pdt_ffp.h"
#include "pdt_tone.h"

static_assert(sizeof(pdt_ffp_sync) == sizeof(pdt::FfpSync) && sizeof(pdt_ffp_sync) == 72, "pdt_ffp_sync");
static_assert(sizeof(pdt_ffp_block) == sizeof(pdt::FfpBlock) && sizeof(pdt_ffp_block) == 40, "pdt_ffp_block");
static_assert(sizeof(pdt_ffp_cfg) == 32, "pdt_ffp_cfg");

namespace pdt {

// One call, as the kernels see it (passed by value)
struct FfpCall {
    const float *y;                 // the stream, n pairs
    float *v;                       // the mixed stream, n pairs (scratch)
    const uint32_t *steps, *starts; // the mixer's table, nent entries of nfft samples
    long long nent, nfft;
    unsigned long long *metric;     // M(b, tau) at [tau nb + b] (scratch; zero before k_ffp_search)
    FfpBlock *blocks;               // nb records
    unsigned long long *pos;        // nb + 1: the exclusive scan of the counts
    unsigned char *bits;            // '0' / '1'
    float *soft;
    long long *symidx;              // the flywheel kernels' time source: symidx[bitsym[m]] = the sample index of bit m
    unsigned *bitsym;               // = its position
    unsigned long long *nbits;
    FfpSync *sync;
    FfpSync head;                   // the record but for nbits, filled on the host
    FfpRule r;
    long long bit_cap;
    int S, TG, chunks, groups;      // k_ffp_search's tiling: own bits per workgroup, hypotheses per workgroup, and how many of each a block has
};

// A workgroup's LDS (the kernels) or a piece of heap (a host walk through the same steps): v's staged piece, the (c, e) pairs of nj bits
// of ng hypotheses at [j ng + g], and per hypothesis its offset, the bit of j = 0, the bits that exist, the start of its first own bit,
// the number of its own bits (own bit k is j = k + W) and its metric
struct FfpTile {
    float2 *piece;
    float4 *ce;
    long long *off, *m0, *lo, *hi, *xs, *own;
    unsigned long long *acc;
};
constexpr int FFP_TILE_HYP = 64;
__host__ __device__ inline size_t ffp_tile_bytes(int ng, int nj) { return (size_t)FFP_PIECE * 8 + (size_t)ng * (size_t)nj * 16 + 7 * FFP_TILE_HYP * 8; }
__host__ __device__ inline FfpTile ffp_tile_at(void *p, int ng, int nj)
{
    FfpTile t;
    unsigned char *q = (unsigned char *)p;
    t.piece = (float2 *)q;
    q += (size_t)FFP_PIECE * 8;
    t.ce = (float4 *)q;
    q += (size_t)ng * (size_t)nj * 16;
    long long *a = (long long *)q;
    t.off = a;
    t.m0 = a + FFP_TILE_HYP;
    t.lo = a + 2 * FFP_TILE_HYP;
    t.hi = a + 3 * FFP_TILE_HYP;
    t.xs = a + 4 * FFP_TILE_HYP;
    t.own = a + 5 * FFP_TILE_HYP;
    t.acc = (unsigned long long *)(a + 6 * FFP_TILE_HYP);
    return t;
}

// bits of one piece: the samples of (bits + 1) bits and the slack of ffp_piece_range fit FFP_PIECE
__host__ __device__ inline int ffp_piece_bits(long long fs) { return (int)((FFP_PIECE - 4) / ((2 * fs + 16639) / 16640)) - 1; }

// hypothesis g of a tile: offset `off`, first own bit `first`, `own` own bits
__host__ __device__ inline void ffp_tile_hyp(const FfpTile &t, int g, const FfpRule &r, long long off, long long first, long long own)
{
    t.off[g] = off;
    t.m0[g] = first - r.W;
    ffp_exist(r.n, off, r.fs, t.lo[g], t.hi[g]);
    t.xs[g] = ffp_t(2 * first, r.fs) + off;
    t.own[g] = own;
    t.acc[g] = 0;
}

// The samples the bits j0 <= j < j1 of every hypothesis of a tile lie in, [s0, s1]: the first own bits start within one bit (and 3 / 65536
// sample) of xmin, the smallest start, and t_2(m+j) - t_2m lies within 1 / 65536 sample of j bits
__host__ __device__ inline void ffp_piece_range(long long xmin, int W, int j0, int j1, long long fs, long long &s0, long long &s1)
{
    s0 = ffp_floordiv(xmin + ffp_floordiv((long long)(j0 - W) * fs * 512, 65) - 2, 65536);
    s1 = ffp_floordiv(xmin + ffp_ceildiv((long long)(j1 + 1 - W) * fs * 512, 65) + 5, 65536);
}

// lane tid of nt: its share of the piece [s0, s1] of v, zeros outside the stream
__host__ __device__ inline void ffp_stage(const FfpTile &t, const float *__restrict__ v, long long n, long long s0, long long s1, int tid, int nt)
{
    const float2 *__restrict__ vv = reinterpret_cast<const float2 *>(v);
    const int len = (int)(s1 - s0 + 1);
    for (int i = tid; i < len && i < FFP_PIECE; i += nt) {
        const long long idx = s0 + i;
        t.piece[i] = idx >= 0 && idx < n ? vv[idx] : make_float2(0.0f, 0.0f);
    }
}

// lane tid of nt: its share of the (c, e) pairs of the bits j0 <= j < j1 of ng hypotheses, from the staged piece that begins at sample s0;
// consecutive lanes take consecutive hypotheses of one j, whose samples lie side by side.  A bit that does not exist, or that no own bit's
// window reaches, is a pair of zeros
__host__ __device__ inline void ffp_pairs(const FfpTile &t, const FfpRule &r, int ng, int j0, int j1, long long s0, int tid, int nt)
{
    const int items = (j1 - j0) * ng;
    for (int it = tid; it < items; it += nt) {
        const int j = j0 + it / ng, g = it % ng;
        const long long m = t.m0[g] + j;
        float4 o = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        if (j < t.own[g] + 2 * r.W && m >= t.lo[g] && m <= t.hi[g])
            ffp_bit(reinterpret_cast<const float *>(t.piece), s0, m, t.off[g], r.fs, o.x, o.y, o.z, o.w);
        t.ce[(size_t)j * ng + g] = o;
    }
}

// d of own bit k of hypothesis g: the window's chain over the pairs, then the cross product
__host__ __device__ inline float ffp_decide(const FfpTile &t, int ng, int W, int k, int g)
{
    float rr = 0.0f, ri = 0.0f;
    for (int w = 0; w <= 2 * W; w++) {
        const float4 c = t.ce[(size_t)(k + w) * ng + g];
        rr += c.x;
        ri += c.y;
    }
    const float4 e = t.ce[(size_t)(k + W) * ng + g];
    return ff_cross(e.z, e.w, rr, ri);
}

__host__ __device__ inline long long ffp_tile_xmin(const FfpTile &t, int ng)
{
    long long x = t.xs[0];
    for (int g = 1; g < ng; g++) x = t.xs[g] < x ? t.xs[g] : x;
    return x;
}
__host__ __device__ inline long long ffp_tile_most(const FfpTile &t, int ng)
{
    long long x = 0;
    for (int g = 0; g < ng; g++) x = t.own[g] > x ? t.own[g] : x;
    return x;
}

// what workgroup (b, chunk, group) of k_ffp_search sets up for hypothesis g < ng of its group
__host__ __device__ inline void ffp_search_hyp(const FfpTile &t, const FfpCall &c, long long b, int chunk, int grp, int g)
{
    const FfpRule &r = c.r;
    const long long off = ffp_off(grp * c.TG + g, r.fs, r.T);
    const long long first = ffp_first_bit((b * r.L) << 16, off, r.fs), next = ffp_first_bit(((b + 1) * r.L) << 16, off, r.fs);
    long long lo, hi;
    ffp_exist(r.n, off, r.fs, lo, hi);
    const long long mine = first + (long long)chunk * c.S, end = next < hi + 1 ? next : hi + 1;
    long long own = end - mine;
    own = own < 0 ? 0 : own > c.S ? c.S : own;
    ffp_tile_hyp(t, g, r, off, mine, own);
}

#if defined(__HIP_DEVICE_COMPILE__)
#define FFP_LDS_ADD(p, x) atomicAdd((p), (x))
#else
#define FFP_LDS_ADD(p, x) (*(p) += (x))
#endif

// lane tid of nt: q(d) of its share of the own bits, into the hypotheses' metrics
__host__ __device__ inline void ffp_search_sum(const FfpTile &t, const FfpRule &r, int ng, long long most, int tid, int nt)
{
    const long long items = most * ng;
    for (long long it = tid; it < items; it += nt) {
        const int k = (int)(it / ng), g = (int)(it % ng);
        if (k >= t.own[g]) continue;
        const unsigned long long q = ff_quant(ffp_decide(t, ng, r.W, k, g));
        if (q) FFP_LDS_ADD(&t.acc[g], q);
    }
}

// block b of k_ffp_track's first step: Ms(b, .), its arg-max and the metric there
__host__ __device__ inline void ffp_track_pick(const FfpCall &c, long long b)
{
    const FfpRule &r = c.r;
    const long long b0 = b - r.J < 0 ? 0 : b - r.J, b1 = b + r.J > r.nb - 1 ? r.nb - 1 : b + r.J;
    unsigned long long best = 0;
    int tau = 0;
    for (int t = 0; t < r.T; t++) {
        unsigned long long s = 0;
        for (long long k = b0; k <= b1; k++) s += c.metric[(size_t)t * (size_t)r.nb + (size_t)k];
        if (s > best) {
            best = s;
            tau = t;
        }
    }
    c.blocks[b].tau = tau;
    c.blocks[b].metric = best;
    c.blocks[b].reserved_ = 0;
}

// delta_b, tau_0 for block 0
__host__ __device__ inline long long ffp_track_delta(const FfpCall &c, long long b)
{
    return b ? (long long)ffp_fold(c.blocks[b].tau, c.blocks[b - 1].tau, c.r.T) : (long long)c.blocks[0].tau;
}

// m_lo(b) under phi
__host__ __device__ inline long long ffp_track_lo(const FfpRule &r, long long b, long long phi)
{
    return ffp_first_bit((b * r.L) << 16, ffp_off(phi, r.fs, r.T), r.fs);
}

// the count of block b once every phi is known; leaves first_bit
__host__ __device__ inline unsigned long long ffp_track_count(const FfpCall &c, long long b)
{
    const FfpRule &r = c.r;
    const long long phi = c.blocks[b].phi, lo = ffp_track_lo(r, b, phi), end = ffp_last_bit(r.n, ffp_off(phi, r.fs, r.T), r.fs) + 1;
    long long hi = end;
    if (b + 1 < r.nb) {
        const long long nx = ffp_track_lo(r, b + 1, c.blocks[b + 1].phi);
        hi = nx < end ? nx : end;
    }
    c.blocks[b].first_bit = lo;
    return hi > lo ? (unsigned long long)(hi - lo) : 0ull;
}

// own bit k of a tile of k_ffp_bits (one hypothesis) to position p of the outputs
__host__ __device__ inline void ffp_emit(const FfpTile &t, const FfpCall &c, int k, long long m, unsigned long long p)
{
    if ((long long)p >= c.bit_cap) return;
    const float d = ffp_decide(t, 1, c.r.W, k, 0);
    c.bits[p] = d > 0.0f ? '1' : '0';
    c.soft[p] = ff_soft(d);
    c.symidx[p] = ffp_end_sample(m, t.off[0], c.r.fs);
    c.bitsym[p] = (unsigned)p;
}

// One workgroup per tile of FFP_MIX_TILE samples: v[i] = y[i] e^{-j 2 pi phase(i) / 2^32}, the segment's step and start phase from the table.
__global__ void __launch_bounds__(256) k_ffp_mix(const FfpCall c, const float *__restrict__ tab)
{
    const long long base = (long long)blockIdx.x * FFP_MIX_TILE;
    const float2 *__restrict__ y = reinterpret_cast<const float2 *>(c.y);
    float2 *__restrict__ v = reinterpret_cast<float2 *>(c.v);
#pragma unroll
    for (int j = 0; j < FFP_MIX_TILE / 256; j++) {
        const long long i = base + 256 * j + (int)threadIdx.x;
        if (i < c.r.n) {
            const float2 a = y[i];
            float2 o;
            ddc_mix(a.x, a.y, ffp_phase(c.steps, c.starts, c.nent, c.nfft, i), tab, o.x, o.y);
            v[i] = o;
        }
    }
}

// The hot path.  A workgroup takes one block, one chunk of at most S of its bits and one group of at most TG clock hypotheses.  Its bits
// with W more on either side are walked in pieces: a piece of v is staged in LDS once (zeros outside the stream) and every sample is
// then used by all hypotheses of the group -- consecutive lanes take consecutive hypotheses of one bit, whose samples lie side by side --
// and the half-bit sums of a hypothesis are formed once: c = h0 + h1 and e = h0 - h1 of every bit stay in LDS.  The reference windows
// are then chains over those c, d = Im(e conj ref), and q(d) is an integer: the lanes join it in LDS and the chunks of a block in M by
// integer atomic adds, whatever the order in which anything runs.
__global__ void __launch_bounds__(256) k_ffp_search(const FfpCall c)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char ffp_lds[];
    const FfpRule &r = c.r;
    const int per = c.chunks * c.groups, tid = (int)threadIdx.x, nt = (int)blockDim.x;
    const long long b = (long long)(blockIdx.x / (unsigned)per);
    const int rest = (int)(blockIdx.x % (unsigned)per), chunk = rest / c.groups, grp = rest % c.groups;
    const int ng = r.T - grp * c.TG < c.TG ? r.T - grp * c.TG : c.TG, nj = c.S + 2 * r.W;
    const FfpTile t = ffp_tile_at(ffp_lds, c.TG, nj);
    if (tid < ng) ffp_search_hyp(t, c, b, chunk, grp, tid);
    __syncthreads();
    const long long most = ffp_tile_most(t, ng);
    if (!most) return;
    const long long xmin = ffp_tile_xmin(t, ng);
    const int jn = (int)most + 2 * r.W, step = ffp_piece_bits(r.fs);
    for (int j0 = 0; j0 < jn; j0 += step) {
        const int j1 = j0 + step < jn ? j0 + step : jn;
        long long s0, s1;
        ffp_piece_range(xmin, r.W, j0, j1, r.fs, s0, s1);
        ffp_stage(t, c.v, r.n, s0, s1, tid, nt);
        __syncthreads();
        ffp_pairs(t, r, ng, j0, j1, s0, tid, nt);
        __syncthreads();
    }
    ffp_search_sum(t, r, ng, most, tid, nt);
    __syncthreads();
    if (tid < ng && t.acc[tid]) atomicAdd(c.metric + (size_t)(grp * c.TG + tid) * (size_t)r.nb + (size_t)b, t.acc[tid]);
}

// step 0, a lane per block: Ms, the arg-max.  step 1, one workgroup whose lanes take a run of blocks each: the folded differences and
// their scan to phi, then m_lo, the counts and their scan -- each scan the lanes' own sums, a walk over those in LDS by one lane, and the
// lanes' runs again.  Nothing leaves the device; lane 0 stores the bit count and the record.
__global__ void __launch_bounds__(256) k_ffp_track(const FfpCall c, int step)
{
    __shared__ long long part[256];
    const FfpRule &r = c.r;
    if (step == 0) {
        const long long b = (long long)blockIdx.x * 256 + (int)threadIdx.x;
        if (b < r.nb) ffp_track_pick(c, b);
        return;
    }
    const int tid = (int)threadIdx.x;
    const long long run = (r.nb + 255) / 256, b0 = tid * run < r.nb ? tid * run : r.nb, b1 = b0 + run < r.nb ? b0 + run : r.nb;
    long long s = 0;
    for (long long b = b0; b < b1; b++) s += ffp_track_delta(c, b);
    part[tid] = s;
    __syncthreads();
    if (tid == 0) {
        long long a = 0;
        for (int i = 0; i < 256; i++) {
            const long long x = part[i];
            part[i] = a;
            a += x;
        }
    }
    __syncthreads();
    s = part[tid];
    for (long long b = b0; b < b1; b++) {
        s += ffp_track_delta(c, b);
        c.blocks[b].phi = s;
    }
    __syncthreads();                                                       // (every phi is stored: block b reads phi of b + 1)
    unsigned long long n = 0;
    for (long long b = b0; b < b1; b++) {
        const unsigned long long k = ffp_track_count(c, b);
        c.blocks[b].count = k;
        n += k;
    }
    part[tid] = (long long)n;
    __syncthreads();
    if (tid == 0) {
        long long a = 0;
        for (int i = 0; i < 256; i++) {
            const long long x = part[i];
            part[i] = a;
            a += x;
        }
        const unsigned long long total = (unsigned long long)a < (unsigned long long)c.bit_cap ? (unsigned long long)a : (unsigned long long)c.bit_cap;
        c.pos[r.nb] = (unsigned long long)a;
        *c.nbits = total;
        FfpSync h = c.head;
        h.nbits = total;
        *c.sync = h;
    }
    __syncthreads();
    n = (unsigned long long)part[tid];
    for (long long b = b0; b < b1; b++) {
        c.pos[b] = n;
        n += c.blocks[b].count;
    }
}

// One workgroup per block: the block's own bits under phi_b in rounds of FFP_BITS_CHUNK -- their (c, e) pairs with W more on either side
// through the staged pieces, as in the search, then a bit per lane: d, the character, the soft value and the time source in the layout
// the flywheel's kernels read (bitsym[p] = p, symidx[p] = the sample index).  The count is the device's own.
__global__ void __launch_bounds__(256) k_ffp_bits(const FfpCall c)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char ffp_lds[];
    const FfpRule &r = c.r;
    const int tid = (int)threadIdx.x, nt = (int)blockDim.x;
    const FfpTile t = ffp_tile_at(ffp_lds, 1, FFP_BITS_CHUNK + 2 * r.W);
    const FfpBlock blk = c.blocks[blockIdx.x];
    const unsigned long long at = c.pos[blockIdx.x];
    const long long off = ffp_off(blk.phi, r.fs, r.T);
    const int step = ffp_piece_bits(r.fs);
    for (unsigned long long done = 0; done < blk.count; done += FFP_BITS_CHUNK) {
        const long long own = blk.count - done < FFP_BITS_CHUNK ? (long long)(blk.count - done) : FFP_BITS_CHUNK, first = blk.first_bit + (long long)done;
        __syncthreads();                                                   // (the round before has read its pairs)
        if (tid == 0) ffp_tile_hyp(t, 0, r, off, first, own);
        __syncthreads();
        const int jn = (int)own + 2 * r.W;
        for (int j0 = 0; j0 < jn; j0 += step) {
            const int j1 = j0 + step < jn ? j0 + step : jn;
            long long s0, s1;
            ffp_piece_range(t.xs[0], r.W, j0, j1, r.fs, s0, s1);
            ffp_stage(t, c.v, r.n, s0, s1, tid, nt);
            __syncthreads();
            ffp_pairs(t, r, 1, j0, j1, s0, tid, nt);
            __syncthreads();
        }
        for (int k = tid; k < (int)own; k += nt) ffp_emit(t, c, k, first + k, at + done + (unsigned long long)k);
    }
}

}  // namespace pdt

using namespace pdt;

namespace pdtrt {

// cfg (NULL = all defaults) at sample rate `rate` for a stream of n samples: the rule's constants, whether the residual is the
// caller's.  PDT_ERR_ARG for a rate outside 49920 .. 1064960, n >= 2^36, B outside 64 .. 832, T outside 8 .. 64, W outside 0 .. 64, J
// outside 0 .. 16, an unknown flag or mask bit, a given residual that is not finite or reaches Fs / 2
int ffp_plan(const pdt_ffp_cfg *cfg, uint32_t rate, uint64_t n, FfpRule *r, int *given, double *residual)
{
    if (rate < FFP_MIN_RATE || rate > FFP_MAX_RATE || n >= (uint64_t)FFP_MAX_SAMPLES) return PDT_ERR_ARG;
    r->fs = rate;
    r->n = (long long)n;
    r->B = FFP_B_DEFAULT;
    r->T = FFP_T_DEFAULT;
    r->W = FFP_W_DEFAULT;
    r->J = FFP_J_DEFAULT;
    *given = 0;
    *residual = 0.0;
    if (cfg) {
        if (cfg->zero_mask & ~(uint32_t)(PDT_FFP_ZERO_REF_BITS | PDT_FFP_ZERO_SMOOTH)) return PDT_ERR_ARG;
        if (cfg->flags & ~(uint32_t)PDT_FFP_RESIDUAL_GIVEN) return PDT_ERR_ARG;
        if (cfg->block_bits) r->B = cfg->block_bits;
        if (cfg->clock_steps) r->T = cfg->clock_steps;
        if (cfg->ref_bits || (cfg->zero_mask & PDT_FFP_ZERO_REF_BITS)) r->W = cfg->ref_bits;
        if (cfg->smooth_blocks || (cfg->zero_mask & PDT_FFP_ZERO_SMOOTH)) r->J = cfg->smooth_blocks;
        if (r->B < FFP_B_MIN || r->B > FFP_B_MAX || r->T < FFP_T_MIN || r->T > FFP_T_MAX || r->W < 0 || r->W > FFP_W_MAX || r->J < 0 || r->J > FFP_J_MAX)
            return PDT_ERR_ARG;
        if (cfg->flags & PDT_FFP_RESIDUAL_GIVEN) {
            if (!(std::isfinite(cfg->residual_hz) && fabs(cfg->residual_hz) < 0.5 * (double)rate)) return PDT_ERR_ARG;
            *given = 1;
            *residual = cfg->residual_hz;
        }
    }
    r->L = ffp_block_len(r->B, r->fs);
    r->nb = (r->n + r->L - 1) / r->L;
    return PDT_OK;
}

// room for every bit the blocks can decide: a block holds B bits, the half sample L is rounded by, half a bit of clock step and the
// two ends' rounding
uint64_t ffp_bit_cap(const FfpRule &r) { return (uint64_t)r.nb * (uint64_t)(r.B + 3); }

// The mixer's table from the tone records of the segments at stride nfft (none: one entry of `residual`, the caller's or 0), and the
// record's head
void ffp_steps(const pdt_tone *tones, uint64_t nseg, int nfft, const FfpRule &r, int given, double residual, std::vector<uint32_t> &steps,
               std::vector<uint32_t> &starts, FfpSync *head)
{
    memset(head, 0, sizeof *head);
    head->nblocks = (uint64_t)r.nb;
    head->block_len = r.L;
    head->B = r.B;
    head->T = r.T;
    head->W = r.W;
    head->J = r.J;
    steps.clear();
    starts.clear();
    if (given || !nseg) {
        steps.push_back(ddc_step((double)r.fs, residual));
        starts.push_back(0u);
        head->residual_hz = residual;
        head->step = steps[0];
        head->nfft = given ? 0 : nfft;
        return;
    }
    uint32_t cur = 0, phase = 0;
    bool first = true;
    for (uint64_t j = 0; j < nseg; j++) {
        if (tones[j].valid) {
            cur = ddc_step((double)r.fs, tones[j].residual_hz);
            head->segs_valid++;
            if (first) {
                head->residual_hz = tones[j].residual_hz;
                head->step = cur;
                first = false;
            }
        }
        steps.push_back(cur);
        starts.push_back(phase);
        phase += cur * (uint32_t)nfft;
    }
    head->segs = nseg;
    head->nfft = nfft;
}

// k_ffp_search's tiling for a rule: own bits S and hypotheses TG per workgroup, chunks and groups per block, its LDS bytes
void ffp_tiling(const FfpRule &r, int *S, int *TG, int *chunks, int *groups, size_t *lds)
{
    const int most = r.B + 2;
    int s = most, tg = FFP_CE_BYTES / (16 * (s + 2 * r.W));
    if (tg < FFP_T_MIN) {
        tg = FFP_T_MIN;
        s = FFP_CE_BYTES / (16 * tg) - 2 * r.W;
    }
    if (tg > r.T) tg = r.T;
    const int g = (r.T + tg - 1) / tg;
    tg = (r.T + g - 1) / g;
    *S = s;
    *TG = tg;
    *chunks = (most + s - 1) / s;
    *groups = (r.T + tg - 1) / tg;
    *lds = ffp_tile_bytes(tg, s + 2 * r.W);
}

// the four kernels of a call whose table entries are filled but for the tiling; inner: NULL, or the three events recorded between the
// kernels (CallTimer)
hipError_t ffp_launch(hipStream_t st, FfpCall c, const float *tab_dev, size_t metric_bytes, hipEvent_t *inner)
{
    const FfpRule &r = c.r;
    size_t lds;
    ffp_tiling(r, &c.S, &c.TG, &c.chunks, &c.groups, &lds);
    const long long tiles = (r.n + FFP_MIX_TILE - 1) / FFP_MIX_TILE, groups = r.nb * c.chunks * c.groups;
    if (tiles > 0x7fffffffll || groups > 0x7fffffffll || r.nb > 0x7fffffffll || lds > 64 * 1024) return hipErrorInvalidValue;
    hipError_t e;
    if (metric_bytes && (e = hipMemsetAsync(c.metric, 0, metric_bytes, st)) != hipSuccess) return e;
    if (tiles) hipLaunchKernelGGL(k_ffp_mix, dim3((unsigned)tiles), dim3(256), 0, st, c, tab_dev);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    if (inner && (e = hipEventRecord(inner[0], st)) != hipSuccess) return e;
    if (groups) hipLaunchKernelGGL(k_ffp_search, dim3((unsigned)groups), dim3(256), lds, st, c);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    if (inner && (e = hipEventRecord(inner[1], st)) != hipSuccess) return e;
    if (r.nb) hipLaunchKernelGGL(k_ffp_track, dim3((unsigned)((r.nb + 255) / 256)), dim3(256), 0, st, c, 0);
    hipLaunchKernelGGL(k_ffp_track, dim3(1), dim3(256), 0, st, c, 1);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    if (inner && (e = hipEventRecord(inner[2], st)) != hipSuccess) return e;
    if (r.nb) hipLaunchKernelGGL(k_ffp_bits, dim3((unsigned)r.nb), dim3(256), ffp_tile_bytes(1, FFP_BITS_CHUNK + 2 * r.W), st, c);
    return hipGetLastError();
}

// the call's work buffer: the mixer's table, the mixed stream, the metrics
static size_t ffp_up16(size_t v) { return (v + 15) & ~(size_t)15; }
size_t ffp_work_bytes(const FfpRule &r, size_t nent)
{
    return 2 * ffp_up16(nent * 4) + ffp_up16((size_t)r.n * 8 + 16) + ffp_up16((size_t)r.T * (size_t)r.nb * 8 + 16);
}

// One call: the mixer's table to the device, then the kernels.  The caller ends it with a synchronize (the table of the previous call is
// no longer read: every call ends with one).  hipError as PDT_ERR_NOGPU
int ffp_run_device(hipStream_t st, const float *y, const FfpRule &r, const FfpSync &head, const std::vector<uint32_t> &steps, const std::vector<uint32_t> &starts,
                   const float *tab_dev, void *work, const FfpOutPtrs &out, uint64_t bit_cap, hipEvent_t *inner)
{
    unsigned char *wk = (unsigned char *)work;
    const size_t nent = steps.size(), o_starts = ffp_up16(nent * 4), o_v = 2 * o_starts, o_metric = o_v + ffp_up16((size_t)r.n * 8 + 16),
                 metric_bytes = (size_t)r.T * (size_t)r.nb * 8;
    if (hipMemcpyAsync(wk, steps.data(), nent * 4, hipMemcpyHostToDevice, st) != hipSuccess) return PDT_ERR_NOGPU;
    if (hipMemcpyAsync(wk + o_starts, starts.data(), nent * 4, hipMemcpyHostToDevice, st) != hipSuccess) return PDT_ERR_NOGPU;
    if (hipStreamSynchronize(st) != hipSuccess) return PDT_ERR_NOGPU;          // (the vectors are pageable and the caller's)
    FfpCall c;
    memset(&c, 0, sizeof c);
    c.y = y;
    c.v = (float *)(wk + o_v);
    c.steps = (const uint32_t *)wk;
    c.starts = (const uint32_t *)(wk + o_starts);
    c.nent = (long long)nent;
    c.nfft = head.nfft > 0 ? head.nfft : 1;
    c.metric = (unsigned long long *)(wk + o_metric);
    c.blocks = out.blocks;
    c.pos = out.pos;
    c.bits = out.bits;
    c.soft = out.soft;
    c.symidx = out.symidx;
    c.bitsym = out.bitsym;
    c.nbits = out.nbits;
    c.sync = out.sync;
    c.head = head;
    c.r = r;
    c.bit_cap = (long long)bit_cap;
    return ffp_launch(st, c, tab_dev, metric_bytes, inner) == hipSuccess ? PDT_OK : PDT_ERR_NOGPU;
}

}  // namespace pdtrt

// ---------------------------------------------------------------- the rule on the host, from its text
namespace {

struct HostFfp {
    const float *v;
    FfpRule r;
    // c and e of bit m under off (the bit exists)
    void pair(long long m, long long off, float *ce) const { ffp_bit(v, 0, m, off, r.fs, ce[0], ce[1], ce[2], ce[3]); }
};

// d of every bit lo <= m <= hi that exists under `off`, d[m - lo]
void host_soft(const HostFfp &h, long long off, long long lo, long long hi, std::vector<float> &d)
{
    const long long n = hi - lo + 1;
    std::vector<float> ce((size_t)n * 4);
    for (long long m = lo; m <= hi; m++) h.pair(m, off, &ce[(size_t)(m - lo) * 4]);
    d.resize((size_t)n);
    for (long long m = lo; m <= hi; m++) {
        const long long a = std::max(lo, m - h.r.W), b = std::min(hi, m + h.r.W);
        float rr = 0.0f, ri = 0.0f;
        for (long long k = a; k <= b; k++) {
            rr += ce[(size_t)(k - lo) * 4];
            ri += ce[(size_t)(k - lo) * 4 + 1];
        }
        d[(size_t)(m - lo)] = ff_cross(ce[(size_t)(m - lo) * 4 + 2], ce[(size_t)(m - lo) * 4 + 3], rr, ri);
    }
}

void host_rule(const HostFfp &h, std::vector<FfpBlock> &blocks, std::vector<unsigned char> &bits, std::vector<float> &soft, std::vector<long long> &index)
{
    const FfpRule &r = h.r;
    const size_t nb = (size_t)r.nb;
    std::vector<unsigned long long> M((size_t)r.T * nb, 0ull);
    std::vector<float> d;
    for (int tau = 0; tau < r.T; tau++) {
        const long long off = ffp_off(tau, r.fs, r.T);
        long long lo, hi;
        ffp_exist(r.n, off, r.fs, lo, hi);
        if (hi < lo) continue;
        host_soft(h, off, lo, hi, d);
        for (long long m = lo; m <= hi; m++) {
            const long long start = ffp_t(2 * m, r.fs) + off, b = (start >> 16) / r.L;
            M[(size_t)tau * nb + (size_t)b] += ff_quant(d[(size_t)(m - lo)]);
        }
    }
    blocks.assign(nb, FfpBlock{});
    for (long long b = 0; b < r.nb; b++) {
        unsigned long long best = 0;
        int at = 0;
        for (int tau = 0; tau < r.T; tau++) {
            unsigned long long s = 0;
            for (long long k = std::max(0ll, b - r.J); k <= std::min(r.nb - 1, b + r.J); k++) s += M[(size_t)tau * nb + (size_t)k];
            if (s > best) {
                best = s;
                at = tau;
            }
        }
        blocks[(size_t)b].tau = at;
        blocks[(size_t)b].metric = best;
        blocks[(size_t)b].phi = b ? blocks[(size_t)b - 1].phi + ffp_fold(at, blocks[(size_t)b - 1].tau, r.T) : at;
    }
    bits.clear();
    soft.clear();
    index.clear();
    for (long long b = 0; b < r.nb; b++) {
        FfpBlock &k = blocks[(size_t)b];
        const long long off = ffp_off(k.phi, r.fs, r.T);
        long long lo, hi;
        ffp_exist(r.n, off, r.fs, lo, hi);
        const long long first = ffp_first_bit((b * r.L) << 16, off, r.fs);
        long long end = hi + 1;
        if (b + 1 < r.nb) end = std::min(end, ffp_first_bit(((b + 1) * r.L) << 16, ffp_off(blocks[(size_t)b + 1].phi, r.fs, r.T), r.fs));
        k.first_bit = first;
        k.count = end > first ? (uint64_t)(end - first) : 0;
        if (!k.count) continue;
        // the windows of the block's bits reach W bits either way, as far as bits exist
        const long long a = std::max(lo, first - r.W), z = std::min(hi, end - 1 + r.W);
        std::vector<float> ce((size_t)(z - a + 1) * 4);
        for (long long m = a; m <= z; m++) h.pair(m, off, &ce[(size_t)(m - a) * 4]);
        for (long long m = first; m < end; m++) {
            float rr = 0.0f, ri = 0.0f;
            for (long long q = std::max(a, m - r.W); q <= std::min(z, m + r.W); q++) {
                rr += ce[(size_t)(q - a) * 4];
                ri += ce[(size_t)(q - a) * 4 + 1];
            }
            const float dm = ff_cross(ce[(size_t)(m - a) * 4 + 2], ce[(size_t)(m - a) * 4 + 3], rr, ri);
            bits.push_back(dm > 0.0f ? '1' : '0');
            soft.push_back(ff_soft(dm));
            index.push_back(ffp_end_sample(m, off, r.fs));
        }
    }
}

// the carrier of the rule: the mixer's table and the record's head for a host stream
int host_carrier(uint32_t rate, const float *iq, const FfpRule &r, int given, double residual, std::vector<uint32_t> &steps, std::vector<uint32_t> &starts,
                 FfpSync *head)
{
    std::vector<pdt_tone> tones;
    int got = 0;
    const int nfft = tone_default_nfft((double)rate);
    if (!given && nfft && (uint64_t)r.n >= (uint64_t)nfft) {
        const uint64_t nseg = (uint64_t)r.n / (uint64_t)nfft;
        if (nseg > 0x7fffffffull) return PDT_ERR_ARG;
        tones.resize((size_t)nseg);
        const int rc = pdt_host_tones(rate, 0.0, iq, (uint64_t)r.n, nullptr, tones.data(), (int)nseg, &got);
        if (rc) return rc;
    }
    pdtrt::ffp_steps(tones.data(), (uint64_t)got, nfft, r, given, residual, steps, starts, head);
    return PDT_OK;
}

void host_mix(const float *iq, const FfpRule &r, const std::vector<uint32_t> &steps, const std::vector<uint32_t> &starts, int nfft, float *out)
{
    float tab[2 * AN_TAB];
    analytic_table(tab);
    for (long long i = 0; i < r.n; i++)
        ddc_mix(iq[2 * i], iq[2 * i + 1], ffp_phase(steps.data(), starts.data(), (long long)steps.size(), nfft > 0 ? nfft : 1, i), tab, out[2 * i], out[2 * i + 1]);
}

}  // namespace

extern "C" {

int pdt_host_ffp_mix(uint32_t rate, const float *iq, uint64_t n, const pdt_ffp_cfg *cfg, float *out)
{
    FfpRule r;
    int given;
    double residual;
    if (((!iq || !out) && n) || pdtrt::ffp_plan(cfg, rate, n, &r, &given, &residual)) return PDT_ERR_ARG;
    try {
        std::vector<uint32_t> steps, starts;
        FfpSync head;
        const int rc = host_carrier(rate, iq, r, given, residual, steps, starts, &head);
        if (rc) return rc;
        host_mix(iq, r, steps, starts, head.nfft, out);
    } catch (const std::exception &) { return PDT_ERR_NOMEM; }
    return PDT_OK;
}

int pdt_host_ffp_bits(uint32_t rate, const float *iq, uint64_t n, const pdt_ffp_cfg *cfg, pdt_ffp_sync *sync, uint8_t *bits, float *soft, int64_t *index,
                      uint64_t cap, uint64_t *count, pdt_ffp_block *blocks, uint64_t block_cap)
{
    FfpRule r;
    int given;
    double residual;
    if ((!iq && n) || !sync || !count || pdtrt::ffp_plan(cfg, rate, n, &r, &given, &residual)) return PDT_ERR_ARG;
    try {
        std::vector<uint32_t> steps, starts;
        FfpSync head;
        const int rc = host_carrier(rate, iq, r, given, residual, steps, starts, &head);
        if (rc) return rc;
        std::vector<float> v((size_t)(2 * r.n) + 2);
        host_mix(iq, r, steps, starts, head.nfft, v.data());
        const HostFfp h{ v.data(), r };
        std::vector<FfpBlock> blk;
        std::vector<unsigned char> b;
        std::vector<float> d;
        std::vector<long long> at;
        host_rule(h, blk, b, d, at);
        head.nbits = b.size();
        memcpy(sync, &head, sizeof head);
        const size_t k = (size_t)std::min<uint64_t>(cap, b.size());
        if (bits && k) memcpy(bits, b.data(), k);
        if (soft && k) memcpy(soft, d.data(), k * sizeof(float));
        if (index && k) memcpy(index, at.data(), k * sizeof(int64_t));
        const size_t kb = (size_t)std::min<uint64_t>(block_cap, blk.size());
        if (blocks && kb) memcpy(blocks, blk.data(), kb * sizeof(FfpBlock));
        *count = b.size();
    } catch (const std::exception &) { return PDT_ERR_NOMEM; }
    return PDT_OK;
}

}  // extern "C"
