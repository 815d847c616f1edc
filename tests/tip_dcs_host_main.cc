// tests/tip_dcs_host_main.cc -- TEST INFRASTRUCTURE: the DCS rule's host statement (csrc/pdt_tip_dcs.h) run under the sanitizers on
// heap blocks of their exact size -- the records, the 32 bytes of stream per record, the packets -- so that under -fsanitize=address a read
// outside a record, a segment or the stream, or a write behind the last packet, ends the run.  Each case runs twice: counting only (no
// output array), then into an array of exactly as many packets as were counted; the packets are checked for what the rule promises of
// each one by itself, and their number against the Python model's.  Input: a file of cases, each three uint64 (channel_max, the number of
// records, the number of packets the model found) and the 136-byte records.
#include <stdio.h>
#include <stdlib.h>

#include "../project-desert-tortoise_amd/csrc/pdt_tip_dcs.h"

using namespace pdt;

static_assert(sizeof(TipDcsRec) == 136 && sizeof(TipDcsPacket) == 88 && sizeof(TipDcsSummary) == 80, "layouts");

static int fail(int c, const char *what)
{
    printf("case %d: %s\n", c, what);
    return 1;
}

int main(int argc, char **argv)
{
    FILE *in = argc > 1 ? fopen(argv[1], "rb") : NULL;
    if (!in) {
        printf("usage: %s cases.bin\n", argv[0]);
        return 2;
    }
    int cases = 0;
    uint64_t head[3];
    while (fread(head, 8, 3, in) == 3) {
        const uint64_t n = head[1], want = head[2];
        const unsigned cm = tip_dcs_channel_max((uint32_t)head[0]);
        if (!cm) return fail(cases, "channel_max");
        TipDcsRec *recs = (TipDcsRec *)malloc(n ? n * sizeof *recs : 1);
        uint8_t *S = (uint8_t *)malloc(n ? n * TIP_DCS_SLOTS : 1);
        if (fread(recs, sizeof *recs, n, in) != n) return fail(cases, "short file");
        TipDcsSummary s0, s1;
        const uint64_t found = tip_dcs_host(recs, n, cm, S, NULL, 0, &s0);
        if (found != want || s0.packets != want) return fail(cases, "another number of packets than the model's");
        TipDcsPacket *out = (TipDcsPacket *)malloc(found ? found * sizeof *out : 1);
        if (tip_dcs_host(recs, n, cm, S, out, found, &s1) != found || memcmp(&s0, &s1, sizeof s0)) return fail(cases, "the two runs differ");
        if (s0.used + s0.skipped != n || s0.stream_bytes != s0.used * TIP_DCS_SLOTS || s0.heads != s0.packets + s0.shadowed || s0.complete > s0.packets ||
            s0.doppler_bad > s0.complete || s0.segments > s0.used)
            return fail(cases, "summary");
        uint64_t complete = 0, odd = 0;
        for (uint64_t k = 0; k < found; k++) {
            const TipDcsPacket &P = out[k];
            if (P.frame >= n || P.slot >= TIP_DCS_SLOTS || P.bytes[0] != 0xD6 || P.channel >= cm || P.channel != P.bytes[1]) return fail(cases, "head");
            if (recs[P.frame].bytes[tip_dcs_slot_byte(P.slot)] != 0xD6) return fail(cases, "frame and slot");
            if (P.time != tip_dcs_time(recs[P.frame].time, tip_dcs_slot_byte(P.slot))) return fail(cases, "time");
            const int L = tip_dcs_len(P.bytes[2] >> 4);
            if (!tip_dcs_code_valid(P.bytes[2] >> 4) || P.blocks != tip_dcs_blocks(P.bytes[2] >> 4) || P.nbytes < 3 || P.nbytes > L || P.complete != (P.nbytes == L))
                return fail(cases, "length");
            for (int b = P.nbytes; b < TIP_DCS_MAXLEN; b++)
                if (P.bytes[b]) return fail(cases, "bytes behind the packet");
            if (k && (out[k - 1].frame > P.frame || out[k - 1].stream_index + out[k - 1].nbytes > P.stream_index)) return fail(cases, "order");
            complete += P.complete;
            odd += P.complete && !P.doppler_ok;
        }
        if (complete != s0.complete || odd != s0.doppler_bad) return fail(cases, "counts");
        free(out);
        free(S);
        free(recs);
        cases++;
    }
    fclose(in);
    printf("tip dcs host: ok, %d cases\n", cases);
    return 0;
}
