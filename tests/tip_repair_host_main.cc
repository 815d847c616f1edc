// tests/tip_repair_host_main.cc -- TEST INFRASTRUCTURE: the steps of k_tip_repair (csrc/pdt_tip_repair.h, __host__ __device__) walked on
// the host as the kernel's lanes walk them -- five wavefronts of 64 lanes per record, the ballot as a loop over the lanes, the butterfly
// as six exchange steps, every read in front of the "barrier", every complement one XOR of an aligned 32-bit word behind it -- against
// the rule's host statement tip_repair_host, byte for byte.  The soft values and records live in heap blocks of their exact size, so that
// under -fsanitize=address a read outside [0, n) or outside a record ends the run.  Input: a file of cases, each two uint64 (the number of
// soft values, the number of records), the float32 values, the 136-byte records.
#include <stdio.h>
#include <stdlib.h>

#include <vector>

#include "../project-desert-tortoise_amd/csrc/pdt_tip_repair.h"

using namespace pdt;

static_assert(sizeof(TipRepairRec) == 136 && sizeof(TipRepairInfo) == 52 && sizeof(TipRepairSummary) == 32, "layouts");

static void walk(const float *soft, int64_t n, TipRepairRec *recs, uint64_t count, TipRepairInfo *info, TipRepairSummary *sum)
{
    memset(sum, 0, sizeof *sum);
    for (uint64_t f = 0; f < count; f++) {
        TipRepairRec *r = recs + f;
        TipRepairInfo *I = info + f;
        if (!tip_repair_checked(r->complete, r->nbytes, r->bit_index, n)) {
            for (int g = 0; g < TIP_REPAIR_GROUPS; g++) {
                I->pos[g] = TIP_REPAIR_NONE;
                I->least[g] = 0.0f;
                I->next[g] = 0.0f;
            }
            I->status = 0;
            I->failed = 0;
            sum->skipped++;
            continue;
        }
        const float *soft0 = soft + (r->bit_index - TIP_REPAIR_LEAD);
        unsigned s_failed[TIP_REPAIR_GROUPS];
        int word[TIP_REPAIR_GROUPS];
        uint32_t mask[TIP_REPAIR_GROUPS];
        for (int g = 0; g < TIP_REPAIR_GROUPS; g++) {                       // in front of the barrier: one wavefront per group
            TipRepairPair best[64], next[64];
            unsigned long long ballot = 0;
            for (int lane = 0; lane < 64; lane++) {
                best[lane] = tip_repair_lane(soft0, g, lane);
                const unsigned odd = lane < 17 ? tip_repair_byte_odd(r->bytes, g, lane) : lane == 17 ? tip_repair_parity_bit(r->bytes, g) : 0u;
                ballot |= (unsigned long long)odd << lane;
            }
            const bool failed = __builtin_popcountll(ballot) & 1;
            for (int d = 32; d >= 1; d >>= 1) {
                for (int lane = 0; lane < 64; lane++) next[lane] = tip_repair_merge(best[lane], best[lane ^ d]);
                memcpy(best, next, sizeof best);
            }
            for (int lane = 1; lane < 64; lane++)
                if (best[lane].lo != best[0].lo || best[lane].hi != best[0].hi) {
                    printf("record %llu group %d: lane %d ends with another pair than lane 0\n", (unsigned long long)f, g, lane);
                    exit(1);
                }
            s_failed[g] = failed ? 1u << g : 0u;
            const int j = (int)(best[0].lo & 0xffffu);
            I->pos[g] = failed ? (uint16_t)j : TIP_REPAIR_NONE;
            I->least[g] = tip_repair_float(best[0].lo);
            I->next[g] = tip_repair_float(best[0].hi);
            word[g] = tip_repair_word(j);
            mask[g] = tip_repair_mask(j);
        }
        for (int g = 0; g < TIP_REPAIR_GROUPS; g++) {                       // behind it: the complements, a word at a time
            if (!s_failed[g]) continue;
            if (word[g] < 0 || word[g] >= (int)(sizeof(TipRepairRec) / 4)) {
                printf("record %llu group %d: word %d outside the record\n", (unsigned long long)f, g, word[g]);
                exit(1);
            }
            uint32_t w;
            memcpy(&w, (unsigned char *)r + 4 * word[g], 4);
            w ^= mask[g];
            memcpy((unsigned char *)r + 4 * word[g], &w, 4);
        }
        const unsigned m = s_failed[0] | s_failed[1] | s_failed[2] | s_failed[3] | s_failed[4];
        I->status = 1;
        I->failed = (uint8_t)m;
        sum->checked++;
        if (m) {
            sum->failing++;
            sum->repaired += (uint64_t)__builtin_popcount(m);
        }
    }
}

int main(int argc, char **argv)
{
    FILE *in = argc > 1 ? fopen(argv[1], "rb") : NULL;
    if (!in) {
        printf("usage: %s cases.bin\n", argv[0]);
        return 2;
    }
    int cases = 0;
    uint64_t head[2];
    while (fread(head, 8, 2, in) == 2) {
        const uint64_t n = head[0], count = head[1];
        float *soft = (float *)malloc(n ? n * 4 : 1);
        TipRepairRec *a = (TipRepairRec *)malloc(count ? count * sizeof *a : 1), *b = (TipRepairRec *)malloc(count ? count * sizeof *b : 1);
        TipRepairInfo *ia = (TipRepairInfo *)calloc(count ? count : 1, sizeof *ia), *ib = (TipRepairInfo *)calloc(count ? count : 1, sizeof *ib);
        if (fread(soft, 4, n, in) != n || fread(a, sizeof *a, count, in) != count) {
            printf("case %d: short file\n", cases);
            return 1;
        }
        memcpy(b, a, count * sizeof *a);
        TipRepairSummary sa, sb;
        walk(soft, (int64_t)n, a, count, ia, &sa);
        tip_repair_host(soft, (int64_t)n, b, count, ib, &sb);
        if (memcmp(a, b, count * sizeof *a) || memcmp(ia, ib, count * sizeof *ia) || memcmp(&sa, &sb, sizeof sa)) {
            printf("case %d: the lanes' walk and the rule's statement differ\n", cases);
            return 1;
        }
        free(soft);
        free(a);
        free(b);
        free(ia);
        free(ib);
        cases++;
    }
    fclose(in);
    printf("tip repair host: ok, %d cases\n", cases);
    return 0;
}
