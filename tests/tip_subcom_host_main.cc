// tests/tip_subcom_host_main.cc -- TEST INFRASTRUCTURE: the subcommutation rule's host statement (csrc/pdt_tip_subcom.h) run under the
// sanitizers on heap blocks of their exact size -- the records, the table, the offsets, the cursors, a byte per sample, the samples -- so
// that under -fsanitize=address a read outside a record or the table, or a write behind the last sample, ends the run.  Each case runs
// three times: counting only, into an array of exactly as many samples as were counted, and into one of half as many; the samples are
// checked for what the rule promises of each one by itself, and their number and the spikes' against the Python model's.  Input: a file of
// cases, each six uint64 (records, entries, trusted_only, spike_threshold, the samples and the spikes the model found), the 10-byte
// entries and the 136-byte records; a case of 0 entries takes built-in table number `trusted_only` from the header, trusted_only off.
#include <stdio.h>
#include <stdlib.h>

#include "../project-desert-tortoise_amd/csrc/pdt_tip_subcom.h"

using namespace pdt;

static_assert(sizeof(TipDcsRec) == 136 && sizeof(TipSubcomEntry) == 10 && sizeof(TipSubcomSample) == 24 && sizeof(TipSubcomSummary) == 72, "layouts");

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
    uint64_t head[6];
    while (fread(head, 8, 6, in) == 6) {
        const uint64_t n = head[0], want = head[4], want_spikes = head[5];
        int ne = (int)head[1];
        bool trusted = head[2] != 0;
        const int thr = tip_subcom_threshold((uint32_t)head[3]);
        if (thr < 0) return fail(cases, "threshold");
        TipSubcomEntry *tab;
        if (ne == 0) {
            TipSubcomEntry whole[TIP_SUBCOM_MAX_ENTRIES];
            ne = tip_subcom_builtin((int)head[2], whole);
            if (!ne) return fail(cases, "no such table");
            tab = (TipSubcomEntry *)malloc((size_t)ne * sizeof *tab);
            memcpy(tab, whole, (size_t)ne * sizeof *tab);
            trusted = false;
        } else {
            tab = (TipSubcomEntry *)malloc((size_t)ne * sizeof *tab);
            if (fread(tab, sizeof *tab, (size_t)ne, in) != (size_t)ne) return fail(cases, "short file");
        }
        const int nchan = tip_subcom_table_channels(tab, (uint64_t)ne);
        if (!nchan) return fail(cases, "table");
        TipDcsRec *recs = (TipDcsRec *)malloc(n ? n * sizeof *recs : 1);
        if (fread(recs, sizeof *recs, n, in) != n) return fail(cases, "short file");
        uint64_t *off = (uint64_t *)malloc(((size_t)nchan + 1) * sizeof *off), *cursor = (uint64_t *)malloc((size_t)nchan * sizeof *cursor);
        TipSubcomSummary s0;
        tip_subcom_host_count(recs, n, tab, ne, nchan, trusted, off, &s0);
        const uint64_t found = s0.samples;
        if (found != want || off[nchan] != want) return fail(cases, "another number of samples than the model's");
        if (found > n * (uint64_t)tip_subcom_table_max_fire(tab, ne)) return fail(cases, "more samples than the table can give");
        if (s0.used + s0.skipped + s0.bad_id != n || s0.byte_parity > found || s0.id_parity > found || s0.channels_hit > (uint64_t)nchan) return fail(cases, "summary");
        uint8_t *V = (uint8_t *)malloc(found ? found : 1);
        for (int pass = 0; pass < 3; pass++) {
            const uint64_t cap = pass == 0 ? 0 : pass == 1 ? found : found / 2;
            TipSubcomSample *out = cap ? (TipSubcomSample *)malloc(cap * sizeof *out) : NULL;
            TipSubcomSummary s1 = s0;
            tip_subcom_host_fill(recs, n, tab, ne, nchan, trusted, thr, off, cursor, V, out, cap, &s1);
            if (s1.spikes != want_spikes) return fail(cases, "another number of spikes than the model's");
            s1.spikes = 0;
            if (memcmp(&s0, &s1, sizeof s0)) return fail(cases, "the fill changed the summary");
            uint64_t spikes = 0;
            for (uint64_t k = 0; k < cap; k++) {
                const TipSubcomSample &P = out[k];
                if (P.frame >= n || P.entry >= ne || P.minor_id >= TIP_SUBCOM_CYCLE) return fail(cases, "frame, entry or counter");
                const TipSubcomEntry &E = tab[P.entry];
                const TipDcsRec &R = recs[P.frame];
                if (P.channel != E.channel || P.minor_id != tip_subcom_id(R.bytes) || !tip_subcom_fires(E, P.minor_id)) return fail(cases, "the entry does not fire there");
                if (P.raw != R.bytes[E.byte] || P.value != tip_subcom_value(E, P.raw) || V[k] != P.value) return fail(cases, "value");
                if (P.time != tip_dcs_time(R.time, E.byte)) return fail(cases, "time");
                if ((unsigned)(P.flags & 7) != tip_subcom_flags(E.byte, tip_subcom_failed(R.bytes)) || (trusted && (P.flags & 3))) return fail(cases, "flags");
                if (k < off[P.channel] || k >= off[P.channel + 1]) return fail(cases, "place");
                if (k > off[P.channel] && (out[k - 1].frame > P.frame || (out[k - 1].frame == P.frame && out[k - 1].entry >= P.entry))) return fail(cases, "order");
                for (int b = 0; b < 5; b++)
                    if (P.pad[b]) return fail(cases, "padding");
                spikes += (P.flags & TIP_SUBCOM_SPIKE) != 0;
            }
            if (cap == found && spikes != want_spikes) return fail(cases, "spike flags");
            free(out);
        }
        free(V);
        free(cursor);
        free(off);
        free(recs);
        free(tab);
        cases++;
    }
    fclose(in);
    printf("tip subcom host: ok, %d cases\n", cases);
    return 0;
}
