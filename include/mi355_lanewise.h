/* libmi355_engine.so -- lane-wise reads: compare two registers, or read one, on every lane of an engine in one launch sequence; and the
 * lane-wise write, mi355_lanewise_set_words, which shares their chunks and their scratch.
 *
 * On an engine with lanes (include/mi355_lanes.h) mi355_engine_equal is refused and mi355_lanes_get_words reads one lane: the canonical
 * form of a lane is seven launches and a synchronising read of its flag words, so a comparison on 512 lanes costs thousands of launches.
 * The two entry points below run the same pipeline with the lanes as a grid dimension: one launch sequence and one read per chunk of
 * lanes.  A chunk is as many lanes as keep the pipeline's scratch within 64 MiB (mi355_lanewise_chunk_lanes; at a transform of 8192
 * digits a lane takes about 128 KiB, so 511 lanes); an engine with more lanes takes them chunk by chunk.  The scratch is made at first
 * use.  A lane whose carry chain reports an over-wide digit, and every lane of an engine made under MI355_HOST_CARRY=1, goes through the
 * host carry instead, with the same answer.
 *
 * Pending run carries are folded in first.  Inside a batch (include/mi355_batch.h) the queue runs first, as before every read.  On a handle
 * without lanes, and on a crt handle, there is the one lane 0, answered through mi355_engine_equal / mi355_engine_get_words.
 * mi355_engine_equal itself stays refused on a handle with lanes.
 *
 * Refused, with a message: a null handle or buffer, a count that is not the one stated below, a register index out of range, a register
 * that holds a multiplicand image.
 *
 * Conventions as in mi355_engine.h: 1 = ok, 0 = failure with the message in mi355_engine_last_error(); nothing escapes.
 */
#ifndef MI355_LANEWISE_H
#define MI355_LANEWISE_H

#include "mi355_lanes.h"

#ifdef __cplusplus
extern "C" {
#endif

/* out[l] = 1 when lane l of lhs and lane l of rhs hold the same value mod 2^p - 1 (0 and 2^p - 1 are the same value), else 0.
   count must equal mi355_lanes_count(handle); both registers must hold residues. */
MI355_ENGINE_API int mi355_lanewise_equal(mi355_engine_handle handle, size_t lhs, size_t rhs, uint8_t* out, size_t count);
/* the canonical residue of every lane of src: lane l in words[l * word_count .. (l + 1) * word_count), each what mi355_lanes_get_words
   returns for that lane.  count must equal mi355_lanes_count(handle) * mi355_engine_word_count(handle). */
MI355_ENGINE_API int mi355_lanewise_get_words(mi355_engine_handle handle, size_t src, uint32_t* words, size_t count);
/* The way back: lane l of dst = the residue whose words are words[l * word_count .. (l + 1) * word_count), each as mi355_lanes_set_words
   takes them for that lane (bits at and above p are folded back in, 2^p = 1).  One upload and one launch per chunk of lanes, where lane by
   lane every lane is an upload, a launch and a synchronise.  dst becomes a register of residues on every lane: it may have held a
   multiplicand image or pending run carries.  count must equal mi355_lanes_count(handle) * mi355_engine_word_count(handle).  Under
   MI355_HOST_CARRY=1 the lanes are cut into digits on the host, one by one. */
MI355_ENGINE_API int mi355_lanewise_set_words(mi355_engine_handle handle, size_t dst, const uint32_t* words, size_t count);
/* Informational only: nothing has to be called with its result.  Lanes per chunk for an engine of `lanes` lanes at a transform of
   transform_size digits: the largest count whose scratch, 16 transform_size + 8 ceil(transform_size / 4096) + 64 bytes a lane, fits
   64 MiB; at least 1, at most `lanes`.  It tells a caller how many launch sequences a call above takes and lets the rule be checked
   without a GPU.  Needs no handle. */
MI355_ENGINE_API size_t mi355_lanewise_chunk_lanes(size_t transform_size, size_t lanes);

#ifdef __cplusplus
}
#endif
#endif
