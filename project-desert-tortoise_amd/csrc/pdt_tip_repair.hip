// pdt_tip_repair.hip -- repair of failed TIP parity groups from the soft bit values (pdt_tip_repair.h): the kernel k_tip_repair, its
// launch and the host restatement pdt_host_tip_repair.  A unit of its own, beside pdt_tip_sync.hip.
#include <hip/hip_runtime.h>
#include <exception>
#include <vector>

#include "../../include/pdt.h"
#include "pdt_tip_repair.h"

static_assert(sizeof(pdt_frame) == sizeof(pdt::TipRepairRec) && sizeof(pdt_frame) == 136, "pdt_frame");
static_assert(offsetof(pdt_frame, bytes) == pdt::TIP_REPAIR_BYTES && offsetof(pdt::TipRepairRec, bytes) == pdt::TIP_REPAIR_BYTES, "pdt_frame.bytes");
static_assert(sizeof(pdt_tip_repair_info) == sizeof(pdt::TipRepairInfo) && sizeof(pdt_tip_repair_info) == 52, "pdt_tip_repair_info");
static_assert(sizeof(pdt_tip_repair_summary) == sizeof(pdt::TipRepairSummary) && sizeof(pdt_tip_repair_summary) == 32, "pdt_tip_repair_summary");

namespace pdt {

// One workgroup of five wavefronts per record, one wavefront per parity group; records and groups are independent.  A wavefront's lanes
// take the group's candidates lane, lane + 64 and lane + 128 -- 136 consecutive soft values from an unaligned start and the parity bit's
// -- lanes 0 - 16 the group's bytes; the parity is a popcount of a ballot, the two smallest keys come out of six butterfly steps on the
// 64-bit keys, no LDS in the search.  Every read of the record lies in front of the barrier, every complement behind it, each ONE atomic
// XOR of the aligned 32-bit word that holds the bit: bytes[103] carries all five parity bits, and up to five wavefronts meet in its word.
// nbits: the stream's length on the device (the feed-forward kernels leave it there), read as min(*nbits, bit_cap).
__global__ void __launch_bounds__(320) k_tip_repair(TipRepairRec *__restrict__ recs, unsigned nrec, const float *__restrict__ soft,
                                                    const unsigned long long *__restrict__ nbits, long long bit_cap, TipRepairInfo *__restrict__ info,
                                                    unsigned long long *__restrict__ sum)
{
    __shared__ unsigned s_failed[TIP_REPAIR_GROUPS];
    const unsigned f = blockIdx.x;
    if (f >= nrec) return;
    const int g = (int)(threadIdx.x >> 6), lane = (int)(threadIdx.x & 63);
    const unsigned long long nb = *nbits;
    const long long n = bit_cap <= 0 ? 0 : nb < (unsigned long long)bit_cap ? (long long)nb : bit_cap;
    TipRepairRec *r = recs + f;
    TipRepairInfo *I = info + f;
    const long long p = r->bit_index;
    if (!tip_repair_checked(r->complete, r->nbytes, p, n)) {                       // (the same for every lane of the workgroup)
        if (lane == 0) {
            I->pos[g] = TIP_REPAIR_NONE;
            I->least[g] = 0.0f;
            I->next[g] = 0.0f;
        }
        if (threadIdx.x == 0) {
            I->status = 0;
            I->failed = 0;
            atomicAdd(&sum[1], 1ull);
        }
        return;
    }
    // 18 <= p and p + 813 < n: soft0[16 .. 831] lies in soft[0 .. n)
    const float *soft0 = soft + (p - TIP_REPAIR_LEAD);
    TipRepairPair best = tip_repair_lane(soft0, g, lane);
    const unsigned odd = lane < 17 ? tip_repair_byte_odd(r->bytes, g, lane) : lane == 17 ? tip_repair_parity_bit(r->bytes, g) : 0u;
    const bool failed = __popcll(__ballot(odd)) & 1;
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
        TipRepairPair o;
        o.lo = __shfl_xor(best.lo, d);
        o.hi = __shfl_xor(best.hi, d);
        best = tip_repair_merge(best, o);
    }
    if (lane == 0) s_failed[g] = failed ? 1u << g : 0u;
    __syncthreads();
    if (lane == 0) {
        const int j = (int)(best.lo & 0xffffu);
        I->pos[g] = failed ? (uint16_t)j : TIP_REPAIR_NONE;
        I->least[g] = tip_repair_float(best.lo);
        I->next[g] = tip_repair_float(best.hi);
        if (failed) atomicXor(reinterpret_cast<unsigned *>(r) + tip_repair_word(j), tip_repair_mask(j));
    }
    if (threadIdx.x == 0) {
        const unsigned m = s_failed[0] | s_failed[1] | s_failed[2] | s_failed[3] | s_failed[4];
        I->status = 1;
        I->failed = (uint8_t)m;
        atomicAdd(&sum[0], 1ull);
        if (m) {
            atomicAdd(&sum[2], 1ull);
            atomicAdd(&sum[3], (unsigned long long)__popc(m));
        }
    }
}

}  // namespace pdt

using namespace pdt;

namespace pdtrt {

// the kernel over nrec records that are on the device: one workgroup each.  sum: four zeroed counters (TipRepairSummary)
hipError_t tip_repair_launch(hipStream_t st, void *recs_dev, unsigned nrec, const float *soft_dev, const unsigned long long *nbits_dev, long long bit_cap,
                             void *info_dev, void *sum_dev)
{
    if (!nrec) return hipSuccess;
    hipLaunchKernelGGL(k_tip_repair, dim3(nrec), dim3(320), 0, st, (TipRepairRec *)recs_dev, nrec, soft_dev, nbits_dev, bit_cap, (TipRepairInfo *)info_dev,
                       (unsigned long long *)sum_dev);
    return hipGetLastError();
}

}  // namespace pdtrt

extern "C" {

int pdt_host_tip_repair(const float *soft, uint64_t nbits, pdt_frame *frames, uint64_t n, pdt_tip_repair_info *info, pdt_tip_repair_summary *summary)
{
    if (!summary || (!frames && n) || (!soft && nbits) || n >= (1ull << 31) || nbits >= (1ull << 31)) return PDT_ERR_ARG;
    tip_repair_host(soft, (int64_t)nbits, reinterpret_cast<TipRepairRec *>(frames), n, reinterpret_cast<TipRepairInfo *>(info),
                    reinterpret_cast<TipRepairSummary *>(summary));
    return PDT_OK;
}

}  // extern "C"
