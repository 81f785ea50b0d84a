/*
 * slu_room.h — C ABI of libslu_room.so: reverberation (a room impulse response per row) and additive noise from a bank of
 * recordings at a drawn signal-to-noise ratio, on a batch of waveforms on the device (gfx950 / CDNA4, MI355X).  Both keep
 * every row's length, both are one launch.
 *
 * A fifth, small library next to libslu_hip.so, libslu_decode.so, libslu_intents.so and libslu_resample.so (DESIGN.md
 * section 3 says why it is separate).  Conventions, status codes (slu_status) and the error channel are slu_hip.h's: every
 * failure leaves its message in the calling thread's slu_last_error() of libslu_hip.so, which this library links against
 * for slu::set_error (csrc/slu_common.h), as the other three do.  Data pointers are DEVICE pointers; `stream` is a
 * hipStream_t passed as void*; nothing synchronises, allocates or reads back.  No counterpart in the reference, whose sox
 * chain has neither effect.
 *
 * What both entry points share
 *   len           lengths == NULL: 1 + the index of the row's last non-zero sample (the rule slu_wave_augment states), 0 for
 *                 an all-zero row.  lengths given: lengths[b] clamped into [0, T].
 *   what is read  nothing at or beyond len: a NaN there reaches no output bit (with lengths == NULL the scan for len reads
 *                 the row, and a NaN is a non-zero sample).
 *   tail          y[n] = +0.0f exactly for len <= n < T.  len does not change: a reverberant tail beyond the utterance's
 *                 end is truncated.
 *   determinism   no atomics; the same call twice is bit-equal; row b's result is that of the row run alone (as a batch of
 *                 one row of any width T >= len) with the same choice.
 *   the stream    what is drawn comes from the row's own Philox4x32-10 stream (csrc/slu_philox.h), with the arguments
 *                 slu_wave_augment takes: key = seed; the row's step offset is off = offset + (offset_dev ? *offset_dev : 0)
 *                 + (sub_batch > 0 ? (b / sub_batch) * sub_stride : 0) and its row index bl = sub_batch > 0 ? b % sub_batch
 *                 : b.  Block j (j = 0, 1) of the row is the Philox block with counter
 *                     (blk, off),  blk = 2^63 | j 2^32 | bl                       (ops._philox_block(seed, off, blk) on the host)
 *                 and u(word) = ((float)(word >> 8) + 0.5f) 2^-24, in (0, 1], is slu_wave_augment's aug_uniform.
 *                     block 0 word 0   reverb: applied iff u <= p
 *                     block 0 word 1   reverb: idx = min(n_rirs - 1, (int)((double)u n_rirs))
 *                     block 0 word 2   noise:  applied iff u <= p
 *                     block 0 word 3   noise:  clip j = min(n_clips - 1, (int)((double)u n_clips))
 *                     block 1 word 0   noise:  start s = min(N_j - 1, (int)((double)u N_j))
 *                     block 1 word 1   noise:  snr = snr_lo + u (snr_hi - snr_lo) dB, in fp32, every operation rounded once
 *                 The caller gives the two effects a key of their own (models.ROOM_KEY), so no other draw moves.
 *
 * slu_wave_reverb — per-row FIR, "same" length
 *   in          (B, T) row-major: fp32, or int16 when in_pcm16 != 0 (then the sample is (float)v * in_scale).
 *   lengths     (B) int32 or NULL (above).
 *   banks       (bank_floats) fp32: the impulse responses one behind the other.  The CALLER guarantees finite taps
 *               (slu_hip/room.py RirBank checks them); the library computes no tap.
 *   desc        (n_rirs, 2) int32: offset (in floats), K of each response; it fits when 1 <= K <= 8192, offset >= 0 and
 *               offset + K <= bank_floats.  banks and desc may be NULL when n_rirs == 0.
 *   fixed_idx   (B) int32 or NULL.  Given: row b uses response fixed_idx[b], -1 (any negative value) = none, and nothing is
 *               drawn.  NULL: the choice is drawn (above).
 *   A row whose chosen index is >= n_rirs, or whose descriptor does not fit, is copied as identity; nothing is indexed out
 *   of bounds.
 *   output      for 0 <= n < len:  y[n] = sum_{k = 0}^{min(K - 1, n)} h[k] x[n - k],  k ascending, one fp32 accumulator that
 *               starts at +0 and takes one fmaf per tap: the result does not depend on the tiling, on T or on the batch.
 *               Taps k > n (they would meet x = 0 in front of the row) are not accumulated.
 *   identity    a row without an impulse response is copied bit for bit, PCM16 rows as (float)v * in_scale; +0.0f from len.
 *   out         (B, T) fp32, every element written; must not alias in.
 *   params      (B, 4) fp32 or NULL: applied (1 / 0), idx (the chosen or drawn index, -1 = none), K (0 when not applied), len.
 * One launch: one workgroup of 256 threads per (row, tile of 1024 outputs), four adjacent outputs per thread in registers.
 * The taps are walked in chunks of 1024, k ascending; a chunk's taps and the tile's source window (1024 + 1024 samples) are
 * staged in LDS (12 KB per workgroup) with coalesced 16-byte loads where the row is aligned, PCM16 converted once, zeros
 * outside [0, len).  Chunks whose every tap lies beyond the tile's last valid output are skipped.
 *
 * slu_wave_mix_noise — a segment of a noise recording at a drawn SNR
 *   in          (B, T) fp32;  lengths as above.
 *   noise       (noise_floats) fp32: the clips one behind the other (finite: the caller's guarantee).
 *   ndesc       (n_clips, 2) int32: offset, N of each clip; it fits when N >= 1, offset >= 0 and offset + N <= noise_floats.
 *               A row whose clip is >= n_clips or does not fit is copied.
 *   fixed       (B, 3) 32-bit words or NULL: clip (int32, negative = none), start (int32, taken modulo N), snr (fp32, dB).
 *               Given, it replaces the draws.  NULL: drawn (above) with p, snr_lo, snr_hi.
 *   arithmetic  z[n] = noise[offset_j + (s + n) mod N_j];
 *               Es = (1 / len) sum_{n < len} x[n]^2,  En = (1 / len) sum_{n < len} z[n]^2: both in float64, in a fixed tree
 *               that depends on len alone (thread t of 256 adds the samples 4 c + e, c = t, t + 256, ..., into four float64
 *               accumulators e = 0 .. 3, then (a0 + a1) + (a2 + a3), a 64-lane butterfly and (w0 + w1) + (w2 + w3));
 *               every workgroup of a row recomputes them the same way.
 *               g = (float)sqrt(Es / En * 10^(-snr / 10)) in float64, rounded once; g = 0 when Es == 0 or En == 0 (or len == 0).
 *               y[n] = fmaf(g, z[n], x[n]) for n < len, +0.0f exactly beyond.  A row not applied is copied bit for bit.
 *   out         (B, T) fp32, every element written; must not alias in.
 *   params      (B, 8) fp32 or NULL: applied, clip, start, snr, g, Es, En, len.
 * One launch of B x split workgroups of 256 threads; the split divides the write pass alone and changes no bit.
 *
 * SLU_ERR_INVALID_ARG (both): a NULL pointer that may not be NULL, B outside [1, 65535], T outside [1, 2^31 - 1], n_rirs /
 * n_clips outside [0, 65535], bank_floats / noise_floats outside [0, 2^31 - 1], p outside [0, 1], in_scale, snr_lo or
 * snr_hi not finite, sub_batch negative or no divisor of B, out == in — the message names the argument.  All refusals
 * happen before any launch.
 */
#ifndef SLU_ROOM_H
#define SLU_ROOM_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SLU_ROOM_ABI_VERSION 1

int slu_wave_reverb(const void* in, int in_pcm16, float in_scale, int64_t B, int64_t T, const int32_t* lengths,
                    const float* banks, int64_t bank_floats, const int32_t* desc, int64_t n_rirs, const int32_t* fixed_idx,
                    float p, uint64_t seed, uint64_t offset, const uint64_t* offset_dev, int64_t sub_batch,
                    uint64_t sub_stride, float* out, float* params, void* stream);
int slu_wave_mix_noise(const float* in, int64_t B, int64_t T, const int32_t* lengths, const float* noise,
                       int64_t noise_floats, const int32_t* ndesc, int64_t n_clips, const void* fixed, float p, float snr_lo,
                       float snr_hi, uint64_t seed, uint64_t offset, const uint64_t* offset_dev, int64_t sub_batch,
                       uint64_t sub_stride, float* out, float* params, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* SLU_ROOM_H */
