/* libmi355_engine.so -- batches: a run of register operations of a one-launch engine as one launch.
 *
 * On an engine created with the plan token onelaunch (include/mi355_lanes.h; any lane count, 1 included) a lane lives entirely inside one
 * work-group, so a whole sequence of register operations can run in one launch: every work-group walks the sequence for its own lanes.
 * Between mi355_batch_begin and mi355_batch_end
 *   - mi355_engine_copy, add, sub_reg, addsub, addsub_copy,
 *   - every product the token makes one launch: square_mul, prepare, mul, mul_add (add_src == dst too), mul_copy, square_mul_copy,
 *     mul_sum where it is one product, square_mul_prepare, with factors up to the plan's fused bound,
 *   - the loops of square_mul_n (sub == 0) and square_mul_bits
 * check their arguments and keep the engine's books at the call, as always, and are then queued instead of launched.  The queue runs, in
 * order, as one launch when the batch ends, when it is full (it then goes on filling), or when anything else is asked of the engine:
 * sub_u32, factors above the fused bound, set_*, every read, sync, equal, raw images.  Those run behind the queue as they do without a
 * batch.  Results are those of the same calls issued one by one: digits and pending carries bit for bit, multiplicand images as the same
 * field elements in the same order.  A call that is refused fails at the call, as without a batch; what was queued before it still runs.
 * Destroying an engine with a batch open discards what is queued.
 *
 * Refused, with a message that names `batch`: mi355_batch_begin on an engine without the token onelaunch or on a "crt..." engine, a second
 * mi355_batch_begin, mi355_batch_end without a batch.  Batching is never chosen by itself.
 *
 * Conventions as in mi355_engine.h: 1 = ok, 0 = failure with the message in mi355_engine_last_error(); nothing escapes.
 */
#ifndef MI355_BATCH_H
#define MI355_BATCH_H

#include "mi355_engine.h"

#ifdef __cplusplus
extern "C" {
#endif

/* from here on the operations listed above are queued */
MI355_ENGINE_API int mi355_batch_begin(mi355_engine_handle handle);
/* runs what is queued and ends the batch (the batch is ended even when the launch fails) */
MI355_ENGINE_API int mi355_batch_end(mi355_engine_handle handle);
/* out[0]: operations queued since the engine was made, out[1]: batch launches since then, out[2]: capacity of the queue in operations,
   out[3]: operations queued and not yet launched.  All zero on an engine that has no batches. */
MI355_ENGINE_API int mi355_batch_stats(mi355_engine_handle handle, uint64_t out[4]);

#ifdef __cplusplus
}
#endif
#endif
