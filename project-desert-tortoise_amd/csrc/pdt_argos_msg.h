// pdt_argos_msg.h -- who sent what: the ARGOS messages in a stream of Manchester bits.  The reference frames an ARGOS
// burst with one 13-bit word, upright only: it sees one-block messages of one polarity.  A platform sends 1 .. 8 blocks of 32 bits
// behind a 20-bit ID, and a receiver whose spectrum is mirrored (or whose I and Q are swapped) delivers every bit complemented.  There
// is no reference to be bit-exact against, so the rule is fixed here, once, for the kernels (pdt_argos_msg.hip) and their host
// restatement (pdt_host_argos_messages) alike:
//   b[i]   = bit i of the stream: a byte of PDT_ST_BITS other than '0' is a one (as in k_sync_hits)
//   c[i]   = b[i] XOR p for a polarity p in {0, 1}
//   a HEAD ends at bit e when
//     sync         c[e-12 .. e-4] = 0 0 0 1 0 1 1 1 1          (the frame sync 00010111 and the initialisation bit 1)
//     length code  c[e-3 .. e]    = N - 1 in three bits, then an even-parity bit: 0000 0011 0101 0110 1001 1010 1100 1111 for N = 1 .. 8;
//                                   the other eight codes are no head
//     run          the K RAW bits b[e-12-K .. e-13] are all equal, EITHER value (K = min_run, 0 .. 15, default 6; 0: no run asked for).
//                  They are the end of the 15 bit-sync ones, 10 10 10 .. in Manchester symbols: until the first data transition the
//                  decoder's pairing of symbols is arbitrary, so the run comes out as ones or as zeros whatever the message's polarity
//     start        e >= 12 + K: bits in front of the stream do not exist (the reference's ring of zeros has no counterpart here)
//   at most one polarity can match at a given e (the sync of one is not the complement of itself)
//   the BODY is c[e+1 .. e+20+32 N]: id = the first 20 bits, MSB first; data = the other 32 N bits, MSB first, in 4 N bytes;
//     complete = the stream holds all of them, else data_bits = the data bits present and the missing bits are 0
//   heads are taken in ascending e; one is accepted only if its first sync bit e - 12 lies behind the last bit e' + 20 + 32 N' of the
//     message accepted before it.  Rejected heads leave no trace.
//   run_value = c[e-13], the run as the message's polarity reads it: 1 = the bit-sync ones came out as ones (0 when K = 0)
//   bit_index = e; time_src and time are those of a pdt_frame whose sync word completes at bit e (symidx[bitsym[e]])
// 28-bit IDs cannot be told from 20-bit ones without the platform registry: out of scope, the first 8 data bits of such a platform's
// message are the rest of its ID.
//
// The text above is rule 0, PDT_ARGOS_RULE_FIRST, the default.  Rule 1, PDT_ARGOS_RULE_BEST, keeps b, p, sync, length code, body, complete
// and the time source and differs in this:
//   run_len(s)   for s in {0, 1}: the number of equal RAW bits that end at b[e-13-s], counted backwards to at most 15 and not past bit 0;
//                0 when bit e-13-s does not exist
//   a HEAD at e  needs the sync and a valid code at e; it takes s = 0 if run_len(0) >= K, otherwise s = 1 if run_len(1) >= K, otherwise it
//                is no head (K = 0: s = 0 always).  The bit b[e-13] of an s = 1 head is a STRAY bit of either value: when the bit-sync ones
//                come out as zeros, the decoder's resync at the first data transition can leave one between the run and the sync.  The
//                test looks at 29 bits; at most one polarity matches at an e
//   score        2 run_len(s) + (1 - s), 0 .. 31;  span = [e - 12, e + 20 + 32 N], the run and the stray bit are not part of it
//   selection    priority: the higher score first, at equal score the smaller e.  A head is accepted if and only if no accepted head of
//                higher priority has a span that overlaps its own (greedy selection in priority order): a false head in the stretch where
//                the loop pulls in has a short run and loses to the true head inside its body.  Records in ascending e; rejected heads
//                leave no trace
//   clusters     heads in ascending e; a head joins the current cluster if its span begins at or before the largest span end seen in that
//                cluster and the cluster holds fewer than ARGOS_CLUSTER_MAX = 256 heads, otherwise it opens a new one.  Selection runs
//                per cluster, the accepted heads of the preceding cluster counting as accepted already (which matters only when the cap
//                closed that cluster: clusters the cap did not cut do not overlap, so apart from the cap this is the global greedy
//                selection).  The cap is part of the rule: it bounds kernel and host alike
//   record       run_value = c[e-13-s], 0 when run_len is 0; reserved_ = run_len | s << 8 (rule 0: 0)
#pragma once
#include <stdint.h>
#include <string.h>

namespace pdt {

constexpr int ARGOS_MSG_TILE = 4096;                       // bits a workgroup of k_argos_msgs packs and tests (pdt_argos_msg_tile())
constexpr int ARGOS_MSG_WORDS = ARGOS_MSG_TILE / 64;
constexpr int ARGOS_MSG_RUN_MAX = 15, ARGOS_MSG_RUN_DEFAULT = 6;
constexpr int ARGOS_MSG_WINDOW = 13 + ARGOS_MSG_RUN_MAX;   // bits a head's test looks at: 28, the window below
constexpr int ARGOS_BEST_WINDOW = ARGOS_MSG_WINDOW + 1;    // ... under rule 1: 29, the stray bit
constexpr int ARGOS_CLUSTER_MAX = 256;                     // heads of a cluster of rule 1
constexpr int ARGOS_RULE_FIRST = 0, ARGOS_RULE_BEST = 1;   // (= PDT_ARGOS_RULE_* of include/pdt.h)

struct ArgosMsg {                   // (= pdt_argos_msg of include/pdt.h)
    double time;
    int64_t bit_index, time_src;
    uint32_t id;
    uint8_t blocks, inverted, complete, run_value;
    uint32_t data_bits;
    uint32_t reserved_;
    uint8_t data[32];
};

struct ArgosCtx {                   // one context of a launch: its bits and their count (device), where its results go
    const unsigned char *bits;
    const unsigned long long *nbits;        // on the device: the chain leaves it there (DevScalars)
    const unsigned *bitsym;                 // bit -> symbol, symbol -> interpolated sample: the frames' time source; NULL: time_src = e
    const long long *symidx;
    unsigned long long *cand;               // the candidate bitmap: bit e & 63 of word e >> 6 = a head ends at e (whole tiles)
    unsigned *tile_any;                     // per tile: its number of heads
    ArgosMsg *out;
    unsigned *count;                        // messages accepted (may exceed cap: the first `cap` are written)
    long long bit_cap;                      // what the buffers hold: the count is read as min(*nbits, bit_cap)
    int cap;
    int first_tile;                         // the context's first workgroup in the launch's grid
};

// A head's test on the window V of the 28 raw bits up to e: bit j of V = b[e - 27 + j] (bit 27 = b[e]; bits in front of the stream: any
// value).  Returns 0: no head; else N | polarity << 4 | run_value << 5.
__host__ __device__ __forceinline__ unsigned argos_head(uint32_t V, long long e, int K)
{
    if (e < 12 + K) return 0;
    const uint32_t sync = (V >> 15) & 0x1ffu;               // bit 0 = b[e-12] .. bit 8 = b[e-4]: 0 0 0 1 0 1 1 1 1 -> 1 1110 1000
    unsigned p;
    if (sync == 0x1e8u) p = 0;
    else if (sync == 0x017u) p = 1;
    else return 0;
    const uint32_t q = ((V >> 24) & 15u) ^ (p ? 15u : 0u);   // bit 0 = c[e-3] (the MSB of N - 1) .. bit 3 = c[e] (the parity)
    const unsigned n1 = ((q & 1u) << 2) | (q & 2u) | ((q >> 2) & 1u), par = (q >> 3) & 1u;
    if ((((n1 >> 2) ^ (n1 >> 1) ^ n1) & 1u) != par) return 0;
    const uint32_t m = (1u << K) - 1u, run = (V >> (15 - K)) & m;
    if (run != 0 && run != m) return 0;
    return (n1 + 1u) | (p << 4) | ((K && (run != 0) != (p != 0)) ? 32u : 0u);
}

// Rule 1: a head's test on the window V of the 29 raw bits up to e: bit j of V = b[e - 28 + j] (bit 28 = b[e]; bits in front of the stream:
// any value).  Returns 0: no head; else N | polarity << 4 | run_value << 5 | run_len << 8 | s << 12 (the low six bits as rule 0's).
__host__ __device__ __forceinline__ unsigned argos_head_best(uint32_t V, long long e, int K)
{
    if (e < 12) return 0;
    const uint32_t sync = (V >> 16) & 0x1ffu;               // bit 0 = b[e-12] .. bit 8 = b[e-4]
    unsigned p;
    if (sync == 0x1e8u) p = 0;
    else if (sync == 0x017u) p = 1;
    else return 0;
    const uint32_t q = ((V >> 25) & 15u) ^ (p ? 15u : 0u);   // bit 0 = c[e-3] (the MSB of N - 1) .. bit 3 = c[e] (the parity)
    const unsigned n1 = ((q & 1u) << 2) | (q & 2u) | ((q >> 2) & 1u), par = (q >> 3) & 1u;
    if ((((n1 >> 2) ^ (n1 >> 1) ^ n1) & 1u) != par) return 0;
    unsigned len[2], val[2];
    for (int s = 0; s < 2; s++) {
        uint32_t r = (V >> (1 - s)) & 0x7fffu;              // bit 14 = b[e-13-s] .. bit 0 = b[e-27-s]
        val[s] = r >> 14;
        if (val[s]) r ^= 0x7fffu;                           // the run as zeros from bit 14 down: its length = 14 - the highest one
        const long long exist = e - 12 - s;                 // bits b[0 .. e-13-s]
        const unsigned n = r ? (unsigned)__builtin_clz(r) - 17u : 15u;
        len[s] = exist <= 0 ? 0u : n < (unsigned long long)exist ? n : (unsigned)exist;
    }
    unsigned s;
    if (K == 0 || len[0] >= (unsigned)K) s = 0;
    else if (len[1] >= (unsigned)K) s = 1;
    else return 0;
    const unsigned rv = len[s] ? val[s] ^ p : 0u;
    return (n1 + 1u) | (p << 4) | (rv << 5) | (len[s] << 8) | (s << 12);
}
__host__ __device__ __forceinline__ unsigned argos_best_run_len(unsigned h) { return (h >> 8) & 15u; }
__host__ __device__ __forceinline__ unsigned argos_best_slip(unsigned h) { return (h >> 12) & 1u; }
__host__ __device__ __forceinline__ unsigned argos_best_score(unsigned h) { return 2u * argos_best_run_len(h) + 1u - argos_best_slip(h); }
// what reserved_ carries under rule 1
__host__ __device__ __forceinline__ uint32_t argos_best_reserved(unsigned h) { return argos_best_run_len(h) | (argos_best_slip(h) << 8); }

// up to 32 bits c[pos .. pos + count), MSB first; bits behind the stream are 0
__host__ __device__ __forceinline__ uint32_t argos_take(const unsigned char *bits, long long nbits, long long pos, int count, unsigned p)
{
    uint32_t v = 0;
    for (int k = 0; k < count; k++) {
        const long long i = pos + k;
        const unsigned char byte = bits[i < nbits ? i : nbits - 1];          // (no branch around the load: the loads of a loop overlap)
        v = (v << 1) | (i < nbits ? ((uint32_t)(byte != '0') ^ p) : 0u);
    }
    return v;
}

// the window of the head test at e, read from the bytes (the finishing pass and the host: the tiles build theirs from packed words)
__host__ __device__ __forceinline__ uint32_t argos_window(const unsigned char *bits, long long e)
{
    uint32_t V = 0;
    for (int j = 0; j < ARGOS_MSG_WINDOW; j++) {
        const long long i = e - (ARGOS_MSG_WINDOW - 1) + j;
        const unsigned char byte = bits[i >= 0 ? i : 0];
        V |= (uint32_t)(i >= 0 && byte != '0') << j;
    }
    return V;
}

// ... and of argos_head_best: 29 bits
__host__ __device__ __forceinline__ uint32_t argos_window_best(const unsigned char *bits, long long e)
{
    uint32_t V = 0;
    for (int j = 0; j < ARGOS_BEST_WINDOW; j++) {
        const long long i = e - (ARGOS_BEST_WINDOW - 1) + j;
        const unsigned char byte = bits[i >= 0 ? i : 0];
        V |= (uint32_t)(i >= 0 && byte != '0') << j;
    }
    return V;
}

// the record of the head `h` = argos_head(..) at e, all but its time stamps
__host__ __device__ __forceinline__ void argos_fill(const unsigned char *bits, long long nbits, long long e, unsigned h, ArgosMsg *m)
{
    const int N = (int)(h & 15u);
    const unsigned p = (h >> 4) & 1u;
    const long long have = nbits - (e + 1);                                   // body bits present
    m->bit_index = e;
    m->id = argos_take(bits, nbits, e + 1, 20, p);
    m->blocks = (uint8_t)N;
    m->inverted = (uint8_t)p;
    m->complete = (uint8_t)(have >= 20 + 32 * N);
    m->run_value = (uint8_t)((h >> 5) & 1u);
    m->data_bits = (uint32_t)(have >= 20 + 32 * N ? 32 * N : have > 20 ? have - 20 : 0);
    m->reserved_ = 0;
    for (int k = 0; k < 8; k++) {
        const uint32_t w = k < N ? argos_take(bits, nbits, e + 21 + 32ll * k, 32, p) : 0u;
        m->data[4 * k] = (uint8_t)(w >> 24);
        m->data[4 * k + 1] = (uint8_t)(w >> 16);
        m->data[4 * k + 2] = (uint8_t)(w >> 8);
        m->data[4 * k + 3] = (uint8_t)w;
    }
}

// the last bit of the body of a message of N blocks whose head ends at e
__host__ __device__ __forceinline__ long long argos_body_end(long long e, int N) { return e + 20 + 32ll * N; }

// The rule on the host, in one pass: out[0 .. min(found, cap)) without time stamps (time_src = bit_index, time = its value); returns found
inline long long argos_host_messages(const unsigned char *bits, long long nbits, int K, ArgosMsg *out, long long cap)
{
    long long found = 0, last_end = -1;
    uint32_t V = 0;
    for (long long e = 0; e < nbits; e++) {
        V = (V >> 1) | ((uint32_t)(bits[e] != '0') << (ARGOS_MSG_WINDOW - 1));
        const unsigned h = argos_head(V, e, K);
        if (!h || e - 12 <= last_end) continue;
        last_end = argos_body_end(e, (int)(h & 15u));
        if (found < cap) {
            ArgosMsg *m = &out[found];
            argos_fill(bits, nbits, e, h, m);
            m->time_src = e;
            m->time = (double)e;
        }
        found++;
    }
    return found;
}

// Rule 1 on the host, in one pass, as argos_host_messages delivers rule 0: a cluster is gathered, resolved by taking the live head of the
// highest priority and striking what overlaps it until none is live, and its winners are appended in ascending e
inline long long argos_host_messages_best(const unsigned char *bits, long long nbits, int K, ArgosMsg *out, long long cap)
{
    long long found = 0, prev_end = -1, cl_end = -1, e_of[ARGOS_CLUSTER_MAX];
    unsigned h_of[ARGOS_CLUSTER_MAX];
    int cl_n = 0;
    auto resolve = [&]() {
        bool live[ARGOS_CLUSTER_MAX], taken[ARGOS_CLUSTER_MAX];
        for (int i = 0; i < cl_n; i++) {
            live[i] = e_of[i] - 12 > prev_end;              // the preceding cluster's accepted heads all lie in front
            taken[i] = false;
        }
        long long ends = -1;
        for (;;) {
            int w = -1;
            for (int i = 0; i < cl_n; i++)
                if (live[i] && (w < 0 || argos_best_score(h_of[i]) > argos_best_score(h_of[w]))) w = i;
            if (w < 0) break;
            const long long wb = e_of[w] - 12, we = argos_body_end(e_of[w], (int)(h_of[w] & 15u));
            for (int i = 0; i < cl_n; i++)
                if (live[i] && e_of[i] - 12 <= we && wb <= argos_body_end(e_of[i], (int)(h_of[i] & 15u))) live[i] = false;
            taken[w] = true;
            if (we > ends) ends = we;
        }
        for (int i = 0; i < cl_n; i++) {
            if (!taken[i]) continue;
            if (found < cap) {
                ArgosMsg *m = &out[found];
                argos_fill(bits, nbits, e_of[i], h_of[i], m);
                m->reserved_ = argos_best_reserved(h_of[i]);
                m->time_src = e_of[i];
                m->time = (double)e_of[i];
            }
            found++;
        }
        prev_end = ends;
        cl_n = 0;
        cl_end = -1;
    };
    uint32_t V = 0;
    for (long long e = 0; e < nbits; e++) {
        V = (V >> 1) | ((uint32_t)(bits[e] != '0') << (ARGOS_BEST_WINDOW - 1));
        const unsigned h = argos_head_best(V, e, K);
        if (!h) continue;
        if (cl_n && (e - 12 > cl_end || cl_n == ARGOS_CLUSTER_MAX)) resolve();
        e_of[cl_n] = e;
        h_of[cl_n] = h;
        cl_n++;
        const long long end = argos_body_end(e, (int)(h & 15u));
        if (end > cl_end) cl_end = end;
    }
    if (cl_n) resolve();
    return found;
}

}  // namespace pdt
