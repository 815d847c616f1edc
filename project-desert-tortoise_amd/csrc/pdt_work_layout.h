// pdt_work_layout.h -- where the regions of the second-pass entries' device buffers lie: offsets only, from counts
// and element sizes, free of HIP, so that tests/work_layout_main.cc walks every layout on the CPU.  The kernels receive pointers into
// these buffers through their tables; none computes one of these offsets itself.  (A braced initialiser evaluates left to right.)
#ifndef PDT_WORK_LAYOUT_H
#define PDT_WORK_LAYOUT_H
#include <stddef.h>

#include <vector>

namespace pdtrt {

// one buffer handed out region by region: every region starts on a 16-byte boundary, `at` is the end of the last one
struct Carve {
    size_t at = 0;
    size_t take(size_t bytes)
    {
        const size_t o = (at + 15) & ~(size_t)15;
        at = o + bytes;
        return o;
    }
};

// ARGOS messages (argos_run): the records and counts of all streams -- [0, o_tab) is read back in one copy --, the table, every
// tile's count and candidate bitmap
struct ArgosWork { size_t o_rec, o_cnt, o_tab, o_any, o_cand, total; };
inline ArgosWork argos_work_layout(size_t streams, size_t recs, size_t tiles, size_t rec_bytes, size_t ctx_bytes, size_t map_bytes)
{
    Carve c;
    return { c.take(recs * rec_bytes), c.take(streams * sizeof(unsigned)), c.take(streams * ctx_bytes), c.take(tiles * sizeof(unsigned)),
             c.take(tiles * map_bytes), c.at };
}

// flywheel synchroniser (tip_sync_run): records, info records and counts -- [0, o_tab) is read back in one copy --, the table, every
// tile's count and offset, six bitmaps of map_bytes each
struct TipSyncWork { size_t o_rec, o_info, o_cnt, o_tab, o_tcnt, o_toff, map_bytes, o_maps, total; };
inline TipSyncWork tip_sync_work_layout(size_t streams, size_t recs, size_t tiles, size_t rec_bytes, size_t info_bytes, size_t ctx_bytes, size_t tile_map_bytes)
{
    Carve c;
    return { c.take(recs * rec_bytes), c.take(recs * info_bytes), c.take(streams * sizeof(unsigned)), c.take(streams * ctx_bytes),
             c.take(tiles * sizeof(unsigned)), c.take(tiles * sizeof(unsigned)), tiles * tile_map_bytes, c.take(6 * tiles * tile_map_bytes), c.at };
}

// feed-forward bits (ff_run): the table and the periods -- [0, o_v) goes up in one copy --, every window's mixed stream of len[i]
// samples (at v[i]), every window's metrics (nr periods, 2H offsets, 8 bytes each; zeroed in one memset), the records side by side
struct FfWork {
    size_t o_tab, o_per, o_v, o_metric, metric_each, o_syncs, total;
    std::vector<size_t> v;
    FfWork(const std::vector<long long> &len, size_t nr, size_t H, size_t win_bytes, size_t sync_bytes)
    {
        Carve c;
        o_tab = c.take(len.size() * win_bytes);
        o_per = c.take(nr * 8);
        o_v = c.take(0);
        for (long long L : len) v.push_back(c.take((size_t)L * 8));
        metric_each = nr * 2 * H * 8;
        o_metric = c.take(len.size() * metric_each);
        o_syncs = c.take(len.size() * sync_bytes);
        total = c.at;
    }
};

// parity repair (tip_repair_run): the counters (64 bytes), the caller's records, their info records
struct RepairWork { size_t o_sum, o_rec, o_info, total; };
inline RepairWork repair_work_layout(size_t recs, size_t rec_bytes, size_t info_bytes)
{
    Carve c;
    return { c.take(64), c.take(recs * rec_bytes), c.take(recs * info_bytes), c.at };
}

// DCS packets (tip_dcs_run): the counters (128 bytes), the records' flags (two spare ones end them), the stream of 32 bytes per record
// rounded up to whole tiles, the head and the bad-code bitmap (a bit per stream byte), every tile's map and entry, the records' time
// stamps or the caller's records (`src_bytes`), the packets
struct DcsWork { size_t o_sum, o_flags, o_stream, o_head, o_bad, o_maps, o_entry, o_src, o_out, total; };
inline DcsWork dcs_work_layout(size_t recs, size_t tiles, size_t tile_bytes, size_t map_bytes, size_t entry_bytes, size_t src_bytes, size_t out_bytes)
{
    Carve c;
    return { c.take(128), c.take(recs + 2), c.take(tiles * tile_bytes), c.take(tiles * tile_bytes / 8), c.take(tiles * tile_bytes / 8),
             c.take(tiles * map_bytes), c.take(tiles * entry_bytes), c.take(src_bytes), c.take(out_bytes), c.at };
}

// subcommutated bytes (tip_subcom_run): the counters (128 bytes) and offsets[0 .. 128] -- [0, o_table) is read back in one copy --, the
// table, a mark per record, every tile's count per channel (channel-major), the records' time stamps or the caller's records
// (`src_bytes`), every possible sample's value (`limit` bytes), the samples
struct SubcomWork { size_t o_sum, o_offsets, o_table, o_marks, o_cnt, o_src, o_vals, o_out, total; };
inline SubcomWork subcom_work_layout(size_t recs, size_t tiles, size_t channels, size_t table_bytes, size_t src_bytes, size_t limit, size_t out_bytes)
{
    Carve c;
    return { c.take(128), c.take(129 * 8), c.take(table_bytes), c.take(recs * sizeof(unsigned)), c.take(channels * tiles * sizeof(unsigned)), c.take(src_bytes),
             c.take(limit), c.take(out_bytes), c.at };
}

// what both feed-forward result buffers end with: time source, soft values, bit -> symbol map and characters of `cap` bits, each over
// the capacity rounded up to 16
struct BitsTail { size_t o_idx, o_soft, o_sym, o_bits; };
inline BitsTail bits_tail(Carve &c, size_t cap)
{
    const size_t r = (cap + 15) & ~(size_t)15;
    return { c.take(8 * r), c.take(4 * r), c.take(4 * r), c.take(r) };
}

// a context's result buffer of the ARGOS feed-forward bits: the count and, at 16, the record (`head` bytes), then the tail
struct FfOut { size_t head; BitsTail t; size_t total; };
inline FfOut ff_out_layout(size_t cap)
{
    Carve c;
    return { c.take(64) + 64, bits_tail(c, cap), c.at };
}

// ... and of the POES ones: count and record, the per-block table, the nb + 1 positions, then the tail; 16 spare bytes end it
struct FfpOut { size_t head, o_blocks, o_pos; BitsTail t; size_t total; };
inline FfpOut ffp_out_layout(size_t nb, size_t cap, size_t block_bytes)
{
    Carve c;
    return { c.take(128) + 128, c.take(nb * block_bytes), c.take((nb + 1) * 8), bits_tail(c, cap), c.at + 16 };
}

}  // namespace pdtrt
#endif
