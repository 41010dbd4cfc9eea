/* libmi355_engine.so -- lanes: many independent residues per register, one launch for all of them.
 *
 * An engine created with the plan token lanes=B,
 *     mi355_engine_create(p, regs, device, verbose, "lanes=64", NULL)        (or "lanes=64,m2=256,c=4")
 * holds B residues mod 2^p - 1 in every register ("lanes") and applies every register operation of include/mi355_engine.h to all of
 * them in one launch: B curves of ECM walk the same ladder on different data.  The handle is an ordinary mi355_engine_handle.
 * B = 1 .. 65535, Goldilocks family only (not with "crt..." specs, not with the split column sweeps); memory is B times that of a plain
 * engine.  What is per register stays per register: whether it holds a residue or a multiplicand image, and every argument check.
 *
 * On a handle with more than one lane
 *   - mi355_engine_set_u32 / set_words / set_digits write every lane; all arithmetic, copy, prepare, sync, describe work on all lanes;
 *   - mi355_engine_get_words / get_digits / res64 / equal / get_data / set_data / get_checkpoint / set_checkpoint / time_square_mul
 *     are refused ("not with lanes"); the four entry points below read and write one lane.
 * On a handle without lanes (and on a crt handle) there is the one lane 0, which is the register itself.
 *
 * The plan token onelaunch ("lanes=512,onelaunch"; p <= 204799, that is a transform of at most 8192 digits) makes every product of the
 * engine -- square_mul, prepare, mul, mul_add, mul_copy, square_mul_copy, mul_sum, square_mul_prepare -- one launch instead of three: a
 * whole lane, front sweep, row sweep and back sweep, runs in one work-group with its work buffer in LDS, and lanes smaller than a
 * work-group share one.  Registers, pending carries and multiplicand images are those of an engine without the token, so every other
 * entry point serves it unchanged; mi355_engine_time_square_mul is refused (there are no phases to time).  It works with any lane count,
 * 1 included (a plain engine with one-launch products), and is refused, with a message that names it, above p = 204799, with c=1, with
 * split5 and on "crt..." specs.  It is never chosen by itself.
 *
 * Conventions as in mi355_engine.h: 1 = ok, 0 = failure with the message in mi355_engine_last_error(); nothing escapes.
 */
#ifndef MI355_LANES_H
#define MI355_LANES_H

#include "mi355_engine.h"

#ifdef __cplusplus
extern "C" {
#endif

/* lanes of the handle: B of its plan token, 1 without one; 0 for a null handle */
MI355_ENGINE_API size_t mi355_lanes_count(mi355_engine_handle handle);
/* one lane of dst = the residue in `words` (word_count little-endian 32-bit words, folded mod 2^p - 1); the other lanes stay as they are.
   Refused when dst holds a multiplicand image: write a value to every lane first (mi355_engine_set_u32). */
MI355_ENGINE_API int mi355_lanes_set_words(mi355_engine_handle handle, size_t lane, size_t dst, const uint32_t* words, size_t count);
/* the canonical residue of one lane of src, in [0, 2^p - 1) */
MI355_ENGINE_API int mi355_lanes_get_words(mi355_engine_handle handle, size_t lane, size_t src, uint32_t* words, size_t count);
/* what mi355_engine_res64 returns for a plain register, for one lane */
MI355_ENGINE_API int mi355_lanes_res64(mi355_engine_handle handle, size_t lane, size_t src, uint64_t* out);

#ifdef __cplusplus
}
#endif
#endif
