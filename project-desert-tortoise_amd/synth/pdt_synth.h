/*
 * pdt_synth.h -- integer-only, counter-based synthetic IQ capture models.
 *
 * Every output sample is a pure function of (parameters, sample index), so a
 * capture can be generated in any order, in parallel, on the host or on the
 * GPU, and is bit-identical everywhere (no floating point after the one-time
 * 65 536-entry sine table, whose CRC is pinned in tests/test_synth.py).
 *
 * Signal models (validated there against the reference decoder):
 *  POES/TIP : s[n] = A exp(j(2 pi f0 n/Fs + phi0 + m d[n])) + w[n], m = 1.06 rad,
 *             d = Manchester symbol (+1/-1) at 16 640 sym/s ('1' -> +1,-1,
 *             '0' -> -1,+1: the inverse of common/ManchesterDecode.c:60-83),
 *             8 320 bit/s, contiguous 104-byte minor frames "ED E2 0b000xxxxx .."
 *             (the 19-bit sync word of POESTIPdemod/main.c:454 is ED E2 + 000),
 *             complex noise 20 dB below the carrier.
 *  ARGOS    : noise floor plus one burst every 1.5 s: 160 ms of unmodulated
 *             carrier, then 400 bit/s Manchester PM (m = 1.1 rad) of
 *             15 x '1', 0001 0111, 1, 0000, 56 payload bits, 1010
 *             (sync "0001011110000": ARGOSdemod/main.c:284), noise 25 dB down.
 *  ARGOS as specified (kind 2): the same bursts with messages of every length: 15 x '1',
 *             0001 0111, 1, the length code of N (N - 1 in three bits and an even-parity
 *             bit), a 20-bit ID, 32 N data bits, then carrier off; N = 1 + (burst + seed)
 *             mod 8, so eight consecutive bursts cover every length (360 .. 920 ms).
 *  POES with parity (kind 3): a POES capture exactly as kind 0 except for byte 103 of every
 *             minor frame: its bit 5 - g is the even parity of bytes 2 + 17 g .. 18 + 17 g, g = 0 .. 4
 *             (the five TIP parity groups); bits 7, 6 and 0 come from the hash as before.
 *  POES with DCS (kind 4): a POES capture exactly as kind 3 except that byte 2 is 8 (NOAA-15), bytes 4 and 5 carry the 9-bit
 *             minor-frame counter fr % 320, and the 32 DCS slots of every frame carry a stream of DCS-2 packets that is a pure
 *             function of the stream byte index (pdt_synth_dcs_stream_byte); the parity bits cover the bytes as sent.
 *
 * A pass as a receiver sees it (round 6; every field 0 = off, the captures above unchanged): noise only before
 * `signal_start` (the receiver is on before the satellite rises) and from `signal_end` on (it stays on after it has set);
 * between the two a linear Doppler ramp -- the carrier's phase step grows by `doppler_q32` / 2^32 per sample, an integer
 * phase accumulator in closed form, so that any sample is still a pure function of its index -- and an amplitude envelope
 * `env_floor_q15` + (1 - floor) 4x(1 - x), x = the position inside the pass: strongest at culmination, `floor` of that at
 * the horizon; and a fade -- `fade_len` samples from `fade_start` at `fade_q15` of that amplitude (an antenna null, a building).
 *
 * All arithmetic is uint32/uint64/int32; phases are 32-bit turns (2^32 = 2 pi).
 */
#ifndef PDT_SYNTH_H
#define PDT_SYNTH_H
#include <stdint.h>

#ifdef __HIPCC__
#define PDT_SYNTH_FN __host__ __device__ static inline
#else
#define PDT_SYNTH_FN static inline
#endif

#define PDT_SYNTH_TABLE_BITS 16
#define PDT_SYNTH_TABLE_SIZE (1u << PDT_SYNTH_TABLE_BITS)

typedef struct pdt_synth_params {
    uint32_t kind;          /* 0 = POES, 1 = ARGOS, 2 = ARGOS with messages of 1 .. 8 blocks, 3 = POES with parity, 4 = POES with parity and DCS */
    uint32_t sample_rate;   /* Hz                                                         */
    uint32_t carrier_step;  /* round(f0 / Fs * 2^32)                                      */
    uint32_t phase0;        /* phi0 in turns * 2^32                                       */
    uint32_t mod_index;     /* m in turns * 2^32                                          */
    int32_t  amplitude;     /* carrier amplitude, int16 units (9830 = 0.3 FS)             */
    int32_t  noise_gain;    /* Q16 multiplier applied to the 4-uniform Irwin-Hall sum     */
    uint64_t seed;          /* payload + noise seed                                       */
    uint64_t signal_start;  /* samples before this index are noise only (carrier off): a  */
                            /* receiver switched on before the satellite rises; 0 = none  */
    uint64_t signal_end;    /* samples from this index on are noise only; 0 = never       */
    int64_t  doppler_q32;   /* carrier_step changes by doppler_q32 / 2^32 per sample      */
                            /* behind signal_start (a linear Doppler ramp); 0 = none      */
    uint32_t env_floor_q15; /* amplitude envelope over [signal_start, signal_end): this   */
                            /* fraction (Q15) at both ends, 1 in the middle; 0 = flat     */
    uint32_t fade_q15;      /* a fade inside the pass: the amplitude times this fraction (Q15)  */
    uint64_t fade_start;    /* ... over the samples [fade_start, fade_start + fade_len); len 0 = */
    uint64_t fade_len;      /* none                                                               */
} pdt_synth_params;

PDT_SYNTH_FN uint64_t pdt_synth_mix(uint64_t z)
{   /* splitmix64 finaliser */
    z += 0x9E3779B97F4A7C15ull;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}

/* byte `b` (0..103) of POES minor frame `fr` */
PDT_SYNTH_FN uint32_t pdt_synth_poes_frame_byte(uint64_t seed, uint64_t fr, uint32_t b)
{
    if (b == 0) return 0xEDu;
    if (b == 1) return 0xE2u;
    uint32_t v = (uint32_t)(pdt_synth_mix(seed ^ (fr * 104u + b) * 0xD6E8FEB86659FD93ull) >> 24) & 0xFFu;
    return b == 2 ? (v & 0x1Fu) : v;
}

/* kind 3: the same, byte 103 carrying the even parity of the five TIP groups in its bits 5 .. 1 */
PDT_SYNTH_FN uint32_t pdt_synth_poes_parity_byte(uint64_t seed, uint64_t fr, uint32_t b)
{
    uint32_t v = pdt_synth_poes_frame_byte(seed, fr, b);
    if (b != 103) return v;
    v &= 0xC1u;
    for (uint32_t g = 0; g < 5; g++) {
        uint32_t x = 0;
        for (uint32_t t = 0; t < 17; t++) x ^= pdt_synth_poes_frame_byte(seed, fr, 2 + 17 * g + t);
        x ^= x >> 4;
        x ^= x >> 2;
        x ^= x >> 1;
        v |= (x & 1u) << (5 - g);
    }
    return v;
}

/* kind 4: the DCS slot 0 .. 31 that frame byte b is (POES.m:869-932: sixteen byte pairs), or -1 */
PDT_SYNTH_FN int pdt_synth_dcs_slot(uint32_t b)
{
    const uint32_t pair = b >> 1;        /* the pairs start at bytes 18 24 28 32 40 44 52 56 60 64 68 72 76 86 90 94 */
    const uint64_t pairs = (1ull << 9) | (1ull << 12) | (1ull << 14) | (1ull << 16) | (1ull << 20) | (1ull << 22) | (1ull << 26) | (1ull << 28) |
                           (1ull << 30) | (1ull << 32) | (1ull << 34) | (1ull << 36) | (1ull << 38) | (1ull << 43) | (1ull << 45) | (1ull << 47);
    if (pair > 47 || !((pairs >> pair) & 1u)) return -1;
    int before = 0;
    for (uint32_t k = 0; k < pair; k++) before += (int)((pairs >> k) & 1u);
    return 2 * before + (int)(b & 1u);
}

/* kind 4: slot group s (64 stream bytes, two frames) holds packet A (which = 0) of 1 + (s + seed) % 8 blocks at its start and packet B
 * (which = 1) of 1 + ((s >> 3) & 1) blocks directly behind it; the rest of the group is zeros */
PDT_SYNTH_FN uint32_t pdt_synth_dcs_blocks(uint64_t seed, uint64_t s, uint32_t which)
{
    return which ? 1u + (uint32_t)((s >> 3) & 1u) : 1u + (uint32_t)((s + seed) & 7u);
}

/* byte j (0 .. 11 + 4 blocks) of that packet: D6, the channel, the length code, the 21-bit time code 2 s + which, four ID bytes, the
 * data, a hashed 23-bit Doppler value with its even-parity bit appended.  An ID or data byte that comes out D6 is sent as D7 */
PDT_SYNTH_FN uint32_t pdt_synth_dcs_packet_byte(uint64_t seed, uint64_t s, uint32_t which, uint32_t j)
{
    const uint32_t n1 = pdt_synth_dcs_blocks(seed, s, which) - 1u, L = 16u + 4u * n1;
    const uint32_t tc = (uint32_t)((2u * s + which) & 0x1FFFFFu);
    if (j == 0) return 0xD6u;
    if (j == 1) return (uint32_t)((s + (which ? 3u : 0u)) & 7u);
    if (j == 2) return ((n1 << 1) | (((n1 >> 2) ^ (n1 >> 1) ^ n1) & 1u)) << 4;
    if (j <= 5) return (tc >> (8u * (5u - j))) & 0xFFu;
    if (j + 3 >= L) {
        uint32_t v = (uint32_t)(pdt_synth_mix(seed ^ ((2u * s + which) * 64u + 63u) * 0x9FB21C651E98DF25ull) >> 24) & 0x7FFFFFu, x = v;
        x ^= x >> 16;
        x ^= x >> 8;
        x ^= x >> 4;
        x ^= x >> 2;
        x ^= x >> 1;
        return (((v << 1) | (x & 1u)) >> (8u * (L - 1u - j))) & 0xFFu;
    }
    const uint32_t v = (uint32_t)(pdt_synth_mix(seed ^ ((2u * s + which) * 64u + j) * 0xA24BAED4963EE407ull) >> 24) & 0xFFu;
    return v == 0xD6u ? 0xD7u : v;
}

/* byte q of the DCS stream: a pure function of the stream byte index */
PDT_SYNTH_FN uint32_t pdt_synth_dcs_stream_byte(uint64_t seed, uint64_t q)
{
    const uint64_t s = q >> 6;
    const uint32_t o = (uint32_t)(q & 63u), la = 12u + 4u * pdt_synth_dcs_blocks(seed, s, 0), lb = 12u + 4u * pdt_synth_dcs_blocks(seed, s, 1);
    if (o < la) return pdt_synth_dcs_packet_byte(seed, s, 0, o);
    if (o < la + lb) return pdt_synth_dcs_packet_byte(seed, s, 1, o - la);
    return 0;
}

/* kind 4: a POES capture as kind 3 whose frames carry a DCS stream: byte 2 is 8 (NOAA-15), bytes 4 and 5 the 9-bit minor-frame counter
 * fr % 320 (byte 4's upper seven bits from the hash as before), the 32 DCS slots the stream above, byte 103 the parity of the bytes as sent */
PDT_SYNTH_FN uint32_t pdt_synth_poes_dcs_data_byte(uint64_t seed, uint64_t fr, uint32_t b)
{
    const int slot = pdt_synth_dcs_slot(b);
    if (slot >= 0) return pdt_synth_dcs_stream_byte(seed, fr * 32u + (uint32_t)slot);
    if (b == 2) return 8u;
    if (b == 4) return (pdt_synth_poes_frame_byte(seed, fr, 4) & 0xFEu) | (uint32_t)((fr % 320u) >> 8);
    if (b == 5) return (uint32_t)((fr % 320u) & 0xFFu);
    return pdt_synth_poes_frame_byte(seed, fr, b);
}
PDT_SYNTH_FN uint32_t pdt_synth_poes_dcs_byte(uint64_t seed, uint64_t fr, uint32_t b)
{
    uint32_t v = pdt_synth_poes_dcs_data_byte(seed, fr, b);
    if (b != 103) return v;
    v &= 0xC1u;
    for (uint32_t g = 0; g < 5; g++) {
        uint32_t x = 0;
        for (uint32_t t = 0; t < 17; t++) x ^= pdt_synth_poes_dcs_data_byte(seed, fr, 2 + 17 * g + t);
        x ^= x >> 4;
        x ^= x >> 2;
        x ^= x >> 1;
        v |= (x & 1u) << (5 - g);
    }
    return v;
}

/* payload byte `b` (0..6) of ARGOS burst `burst` */
PDT_SYNTH_FN uint32_t pdt_synth_argos_payload_byte(uint64_t seed, uint64_t burst, uint32_t b)
{
    return (uint32_t)(pdt_synth_mix(seed ^ (burst * 8u + b + 1u) * 0xA24BAED4963EE407ull) >> 24) & 0xFFu;
}

/* bit `j` (0..87) of an ARGOS burst message */
PDT_SYNTH_FN uint32_t pdt_synth_argos_bit(uint64_t seed, uint64_t burst, uint32_t j)
{
    if (j < 15) return 1;
    if (j < 23) return (0x17u >> (22 - j)) & 1u;         /* 0001 0111 */
    if (j == 23) return 1;
    if (j < 28) return 0;
    if (j < 84) {
        uint32_t k = j - 28;
        return (pdt_synth_argos_payload_byte(seed, burst, k >> 3) >> (7 - (k & 7))) & 1u;
    }
    return (j & 1u) ? 0u : 1u;                            /* 84..87 = 1010 */
}

/* kind 2: the blocks N = 1 .. 8 of burst `burst`, its 20-bit ID, byte `b` (0 .. 4 N - 1) of its data */
PDT_SYNTH_FN uint32_t pdt_synth_argos_blocks(uint64_t seed, uint64_t burst) { return 1u + (uint32_t)((burst + seed) & 7u); }
PDT_SYNTH_FN uint32_t pdt_synth_argos_id(uint64_t seed, uint64_t burst)
{
    return (uint32_t)(pdt_synth_mix(seed ^ (burst * 64u + 33u) * 0xA24BAED4963EE407ull) >> 24) & 0xFFFFFu;
}
PDT_SYNTH_FN uint32_t pdt_synth_argos_data_byte(uint64_t seed, uint64_t burst, uint32_t b)
{
    return (uint32_t)(pdt_synth_mix(seed ^ (burst * 64u + b + 34u) * 0x9FB21C651E98DF25ull) >> 24) & 0xFFu;
}

/* kind 2: bit `j` (0 .. 47 + 32 N) of a burst's message */
PDT_SYNTH_FN uint32_t pdt_synth_argos_msg_bit(uint64_t seed, uint64_t burst, uint32_t j)
{
    if (j < 15) return 1;
    if (j < 23) return (0x17u >> (22 - j)) & 1u;         /* 0001 0111 */
    if (j == 23) return 1;
    if (j < 28) {
        const uint32_t n1 = pdt_synth_argos_blocks(seed, burst) - 1u;
        const uint32_t code = (n1 << 1) | (((n1 >> 2) ^ (n1 >> 1) ^ n1) & 1u);
        return (code >> (27 - j)) & 1u;
    }
    if (j < 48) return (pdt_synth_argos_id(seed, burst) >> (47 - j)) & 1u;
    const uint32_t k = j - 48;
    return (pdt_synth_argos_data_byte(seed, burst, k >> 3) >> (7 - (k & 7))) & 1u;
}

PDT_SYNTH_FN int32_t pdt_synth_noise(uint64_t h, int32_t gain_q16)
{   /* Irwin-Hall(4) of 16-bit uniforms, zero mean, scaled by gain/65536 */
    int32_t s = (int32_t)(h & 0xFFFF) + (int32_t)((h >> 16) & 0xFFFF) + (int32_t)((h >> 32) & 0xFFFF) +
                (int32_t)((h >> 48) & 0xFFFF) - 2 * 65535;
    int64_t v = (int64_t)s * gain_q16;
    return (int32_t)((v + (v >= 0 ? 32768 : -32768)) / 65536);
}

PDT_SYNTH_FN int16_t pdt_synth_clip16(int32_t v)
{
    return (int16_t)(v > 32767 ? 32767 : (v < -32768 ? -32768 : v));
}

/* One IQ sample.  sine_tab[i] = lrint(32767 sin(2 pi i / 65536)). */
PDT_SYNTH_FN void pdt_synth_sample(const pdt_synth_params *p, const int16_t *sine_tab, uint64_t n, int16_t *i_out,
                                   int16_t *q_out)
{
    uint32_t theta = (uint32_t)(n * (uint64_t)p->carrier_step) + p->phase0;
    int32_t amp = n < p->signal_start ? 0 : p->amplitude;
    if (p->signal_end && n >= p->signal_end) amp = 0;
    if (amp && p->doppler_q32) {
        /* sum over the m samples since signal_start of (k * doppler_q32) / 2^32 turns, k = 0 .. m - 1, floor taken of the sum:
           bits 32..63 of the two's complement product doppler_q32 * m (m - 1) / 2 -- its low 64 bits are exact under wrap-around */
        const uint64_t m = n - p->signal_start;
        const uint64_t tri = (m & 1u) ? m * ((m - 1u) >> 1) : (m >> 1) * (m - 1u);
        theta += (uint32_t)(((uint64_t)p->doppler_q32 * tri) >> 32);
    }
    if (amp && p->env_floor_q15 && p->signal_end > p->signal_start) {
        const uint64_t m = n - p->signal_start, len = p->signal_end - p->signal_start;      /* (len < 2^40) */
        const uint64_t x = (m << 16) / len;                                                 /* Q16 position, < 65536 */
        const uint64_t par = 4u * x * (65536u - x);                                         /* Q32: 4x(1 - x) <= 2^32 */
        const uint64_t e = p->env_floor_q15 + (((32768u - (uint64_t)p->env_floor_q15) * par) >> 32);   /* Q15 */
        amp = (int32_t)(((uint64_t)amp * e + 16384u) >> 15);
    }
    if (amp && p->fade_len && n >= p->fade_start && n - p->fade_start < p->fade_len)
        amp = (int32_t)(((uint64_t)amp * p->fade_q15 + 16384u) >> 15);
    if (p->kind == 0 || p->kind == 3 || p->kind == 4) {
        uint64_t k = (n * 16640ull) / p->sample_rate;     /* Manchester symbol index */
        uint64_t bit = k >> 1;
        uint64_t fr = bit / 832u;
        uint32_t j = (uint32_t)(bit % 832u);
        uint32_t v = ((p->kind == 4 ? pdt_synth_poes_dcs_byte(p->seed, fr, j >> 3)
                                    : p->kind == 3 && j >= 824 ? pdt_synth_poes_parity_byte(p->seed, fr, 103) : pdt_synth_poes_frame_byte(p->seed, fr, j >> 3)) >> (7 - (j & 7))) & 1u;
        int up = (v != 0) ^ (int)(k & 1);                 /* '1' -> +,-   '0' -> -,+ */
        theta += up ? p->mod_index : (uint32_t)(0u - p->mod_index);
    } else {
        uint64_t period = (uint64_t)p->sample_rate * 3u / 2u;          /* 1.5 s */
        uint64_t burst = n / period;
        uint64_t off = n % period;
        uint64_t lead = (uint64_t)p->sample_rate * 4u / 25u;           /* 160 ms */
        if (off < lead) {
            /* unmodulated carrier */
        } else {
            uint64_t k = ((off - lead) * 800ull) / p->sample_rate;     /* symbol index */
            const uint64_t nsym = p->kind == 2 ? 2u * (48u + 32u * pdt_synth_argos_blocks(p->seed, burst)) : 176u;
            if (k < nsym) {
                uint32_t v = p->kind == 2 ? pdt_synth_argos_msg_bit(p->seed, burst, (uint32_t)(k >> 1))
                                          : pdt_synth_argos_bit(p->seed, burst, (uint32_t)(k >> 1));
                int up = (v != 0) ^ (int)(k & 1);
                theta += up ? p->mod_index : (uint32_t)(0u - p->mod_index);
            } else {
                amp = 0;                                               /* carrier off */
            }
        }
    }
    const uint32_t idx = theta >> (32 - PDT_SYNTH_TABLE_BITS);
    const int32_t s = sine_tab[idx];
    const int32_t c = sine_tab[(idx + PDT_SYNTH_TABLE_SIZE / 4) & (PDT_SYNTH_TABLE_SIZE - 1)];
    int32_t vi = (amp * c + (1 << 14)) >> 15;
    int32_t vq = (amp * s + (1 << 14)) >> 15;
    vi += pdt_synth_noise(pdt_synth_mix(p->seed ^ (2 * n + 0x51ull) * 0xC2B2AE3D27D4EB4Full), p->noise_gain);
    vq += pdt_synth_noise(pdt_synth_mix(p->seed ^ (2 * n + 0x52ull) * 0xC2B2AE3D27D4EB4Full), p->noise_gain);
    *i_out = pdt_synth_clip16(vi);
    *q_out = pdt_synth_clip16(vq);
}

#ifdef __cplusplus
extern "C" {
#endif
/* host-side helpers (pdt_synth.c) */
const int16_t *pdt_synth_sine_table(void);
void pdt_synth_default_params(pdt_synth_params *p, int kind, uint32_t sample_rate, double f0_hz, uint64_t seed);
/* a pass (round 6): noise only outside [signal_start, signal_end), linear Doppler ramp f_start_hz -> f_end_hz, amplitude envelope */
void pdt_synth_set_pass(pdt_synth_params *p, uint64_t signal_start, uint64_t signal_end, double f_start_hz, double f_end_hz,
                        double env_floor);
/* fill out[2*count] with samples [start, start+count) */
void pdt_synth_fill(const pdt_synth_params *p, uint64_t start, uint64_t count, int16_t *out);
/* canonical 44-byte header (fmt=1, 2 ch, 16 bit) for `nframes` IQ samples */
void pdt_synth_wav_header(uint8_t hdr[44], uint32_t sample_rate, uint64_t nframes);
/* frames / payloads the generator transmitted (for round-trip checks) */
void pdt_synth_poes_frame(const pdt_synth_params *p, uint64_t fr, uint8_t out[104]);
void pdt_synth_argos_payload(const pdt_synth_params *p, uint64_t burst, uint8_t out[7]);
/* kind 2: the message burst `burst` carries -- its blocks, its ID, its 4 N data bytes (the rest of data: 0) */
void pdt_synth_argos_message(const pdt_synth_params *p, uint64_t burst, int *blocks, uint32_t *id, uint8_t data[32]);
/* kind 4: the DCS packet `which` (0 = A, 1 = B) of slot group s as transmitted -- its *len bytes (the rest of out: 0) */
void pdt_synth_dcs_packet(const pdt_synth_params *p, uint64_t s, int which, uint8_t out[44], int *len);
#ifdef __cplusplus
}
#endif
#endif
