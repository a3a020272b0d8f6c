/* fmx_debug.h -- the diagnostic exports of libfmx.  Not part of the drop-in boundary (include/fmx.h): nothing in the reference corresponds
 * to them; bench.py, tools/ and tests/ use them. */
#ifndef FMX_DEBUG_H
#define FMX_DEBUG_H
#include "fmx.h"
#ifdef __cplusplus
extern "C" {
#endif
/* Streaming bandwidth of GPU `device` in GB/s over `bytes` (>= 1 MiB) of float2 data, the mean of `iters` launches timed with HIP events.
 * mode 0: copy (bytes read + written are counted); mode 1: read 12, write 1 -- the input-filter stage's traffic shape; mode 2: the same reads, nothing written (SURVEY 8d asks for the
 * measured device bandwidth beside the nominal 8 TB/s: bench.py `roofline.measured_stream_bandwidth`). */
int fmx_debug_stream_bandwidth(int32_t device, int32_t mode, int64_t bytes, int32_t iters, double *gbps);
/* Per-phase shader-cycle counters of front_kernel (and, in -DSB_FINE_TICKS builds, of stage B), summed over the handle's channels into out[96]
 * (may be null); enable != 0 allocates and clears the counters, 0 frees them.  tools/front_phases.py, tools/stageb_fine.py. */
int fmx_debug_phase_cycles(fmx_handle h, int32_t enable, unsigned long long *out);
/* The scalar state of `channel`'s RDS slicers behind the handle's last call: a plain copy of fields of the device's state records (no launch), the
 * integers as floats; *n = FMX_DEBUG_RDS_STATE_FIELDS, or 0 on a handle whose RDS was never switched on.  capacity >= FMX_DEBUG_RDS_STATE_FIELDS.
 *   [0] rds mode  [1] bits sliced so far
 *   RDS_2  [2] AGC gain  [3] Costas freq  [4] Costas phase  [5] mMu (its fraction)  [6] skip  [7] sampleCount
 *   RDS_1  [8] Costas freq  [9] Costas phase  [10] lastSync
 *   RDS_3  [11] Costas freq  [12] Costas phase  [13] bitClkPhase  [14] sync errors of the block synchroniser  [15] its `synced`
 * tests/test_gpu_rds_slicers.py compares them with the oracle's slicers after every call. */
#define FMX_DEBUG_RDS_STATE_FIELDS 16
int fmx_debug_rds_state(fmx_handle h, int32_t channel, float *out, int32_t capacity, int32_t *n);
#ifdef __cplusplus
}
#endif
#endif
