/* pdt_dev.h -- TEST-ONLY entry of libpdt.so: developer switches.
 *
 * The product never reads the environment.  The A/B switches the tests and the tuning sweeps use (older kernel variants kept as
 * fallbacks for geometries the default kernels do not cover, block geometry overrides, thresholds brought down to test sizes)
 * live in a process-wide registry that only this entry fills; a context copies them once, in pdt_open.  The Python binding the
 * tests and bench.py go through mirrors the process's PDT_* environment variables into it before every pdt_open, so a test
 * still says os.environ["PDT_GSPAN"] = "4"; bin/demodPOES, bin/demodARGOS, bin/demodMulti and any other client of
 * include/pdt.h never call it.  The names are listed in tools/README.md. */
#ifndef PDT_DEV_H
#define PDT_DEV_H
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif
/* value != NULL: set switch `name`; value == NULL: remove it; name == NULL: clear all.  Contexts opened afterwards see it. */
int pdt_dev_set(const char *name, const char *value);
/* (measurement aid, round 6) The boundary-state tables of the last demodulation when their rows span several chunks: the number
 * of rows, and for the first `max` of them the number of DISTINCT exits of the row's first chunk (0xffffffff: a row that was
 * left untabulated).  0 when the last run had no such rows.  What tools/span_hist.py turns into profiles/r6/gardner_row_exits_*.  */
struct pdt_ctx;
unsigned long long pdt_dev_span_rows(const struct pdt_ctx *ctx, unsigned *n_exits_out, unsigned long long max);
/* (measurement aid, round 20) The same rows through the staged span walk: the number of rows, and for the first `max`
 * of them three numbers in out[3 k ...]: the distinct exits of the row's first chunk (as above), the distinct sampler states left
 * at the re-key point, and the stage-2 work items they were cut into.  The last two are 0 for a row that was not staged: the
 * last run had no re-key point (PDT_GSPAN_REKEY=0, a short row), or the row was left untabulated or had too many exits to
 * deduplicate and went through all its chunks in stage 1. */
unsigned long long pdt_dev_span_rekey(const struct pdt_ctx *ctx, unsigned *out, unsigned long long max);
/* Which low-pass filter kernel the last demodulation took (the last segment of a stream): 0 none (no output samples), 1 k_fir_plain
 * (ARGOS), 2 k_mix_fir (mix and filter in one kernel), 3 the register-tiled interpolating form, 4 the generic interpolating
 * form.  *fused_tiles_out (may be NULL): the tile or run maps that kernel wrote for the AGC, 0 when the AGC built its own.  The
 * profile's group is called "fir" whatever was launched; this is how tests/test_gpu_interp.py sees the dispatch. */
unsigned pdt_dev_fir_form(const struct pdt_ctx *ctx, unsigned long long *fused_tiles_out);
/* The down-converter's kernel on ONE record, as a piece of a stream hands it over (csrc/pdt_ddc.h): x_dev is the address of input
 * sample 0 in device memory, the samples lo <= i < hi are present and zeros lie elsewhere, g0 is the global index of input 0
 * (the phase of input i is (g0 + i) step), and outputs 0 <= m < n_out, each centred on input m decim, go to out_dev as float32
 * pairs.  The entry uploads the taps and the rotation table, launches once, waits and frees what it allocated; it has no
 * context.  A stream's converted pairs cannot be read back otherwise: this is how the tests compare a piece with pdt_host_ddc. */
int pdt_dev_ddc(int device, uint32_t in_rate, int decim, double offset_hz, int sample_format, const void *x_dev, long long lo, long long hi,
                uint64_t n_out, uint64_t g0, void *out_dev);
#ifdef __cplusplus
}
#endif
#endif
