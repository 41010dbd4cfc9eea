/* libmi355_engine.so -- across lanes: a product whose multiplicand image comes from another lane.
 *
 * On an engine with lanes (include/mi355_lanes.h) every operation takes all its operands from its own lane, so the lanes cannot be
 * combined on the device: the product of a register over all lanes, and from it every lane's inverse by Montgomery's trick, had to go
 * through the host.  The one entry point below is what that needs.  With
 *
 *     g = ((l >> level) ^ 1) << level        the first lane of lane l's sibling block of 2^level lanes
 *
 * it sets, on every lane l of the engine in one launch sequence,
 *
 *     dst[l] <- dst[l] * src[g]     where g is below the handle's lane count: the image is read from lane g of src
 *     dst[l] <- dst[l] * alt[l]     where g is no lane: the image is read from the own lane of alt
 *
 * dst holds residues (pending run carries allowed); src and alt hold multiplicand images (made by the prepare or square_mul_prepare entry points of
 * mi355_engine.h) and stay as they are; the factor is 1.  Digits, pending carry words and register kind of dst are
 * exactly those of the mul entry point of mi355_engine.h with that image and factor 1.  A caller keeps the image of 1 in alt, so that a lane without
 * a sibling block keeps its value.
 *
 * Use (prmers_amd/lanecross.py): with T a copy of Z and R_s the image of T before level s, levels s = 0 .. L - 1 with
 * L = ceil(log2 lanes) leave the product of Z over ALL lanes in every lane of T, for any lane count; one inversion on the host and the same
 * L products of its result by the R_s give every lane the inverse of its own Z.
 *
 * Inside a batch (include/mi355_batch.h) the queue runs first and the operation is a launch of its own: the image of another lane may be
 * stored by another work-group of the running queue.  On a handle with one lane, plain or crt, no lane has a sibling in range and the
 * operation is the mul of mi355_engine.h on dst and alt with factor 1.
 *
 * Refused, with a message and before anything is launched: a null handle, a register index out of range, dst equal to src or to alt,
 * dst holding a multiplicand image, src or alt not holding one, level above 31.
 *
 * Conventions as in mi355_engine.h: 1 = ok, 0 = failure with the message in the last_error entry point; nothing escapes.
 */
#ifndef MI355_LANECROSS_H
#define MI355_LANECROSS_H

#include "mi355_lanes.h"

#ifdef __cplusplus
extern "C" {
#endif

MI355_ENGINE_API int mi355_lanecross_mul_sibling(mi355_engine_handle handle, size_t dst, size_t src, size_t alt, uint32_t level);

#ifdef __cplusplus
}
#endif
#endif
