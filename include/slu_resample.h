/*
 * slu_resample.h — C ABI of libslu_resample.so: sample-rate conversion of a batch of waveforms on the device (gfx950 /
 * CDNA4, MI355X): a polyphase windowed-sinc rational resampler, every row with its own source rate, PCM16 or fp32 in,
 * fp32 out, length-aware, one launch.
 *
 * A fourth, small library next to libslu_hip.so, libslu_decode.so and libslu_intents.so (DESIGN.md section 3 says why it
 * is separate).  Conventions, status codes (slu_status) and the error channel are slu_hip.h's: every failure leaves its
 * message in the calling thread's slu_last_error() of libslu_hip.so, which this library links against for
 * slu::set_error (csrc/slu_common.h), as the other two do.  Data pointers are DEVICE pointers; `stream` is a hipStream_t
 * passed as void*; nothing synchronises, allocates or reads back.  No counterpart in the reference, whose sox chain has
 * no `rate` effect.
 *
 * Definition (this project's own; the formulas are the ones torchaudio documents for
 * resample(..., resampling_method="sinc_interp_hann") with its defaults, parity with it is not claimed).
 * For a row with source rate fi and the target rate fo:
 *   g = gcd(fi, fo), L = fo / g, M = fi / g;  Z = 6, rolloff = 0.99;
 *   s = rolloff * min(1, L / M)                      the cutoff relative to the source Nyquist frequency
 *   Wd = ceil(Z / s)                                 in source samples
 *   K = 2 Wd + 2 taps, k = -Wd ... Wd + 1
 *   output length   n_out = ceil(len L / M) = (len L + M - 1) / M          (integers)
 *   position        output sample n sits at source position n M / L = q + p / L, q = (n M) / L, p = (n M) % L (64-bit)
 *   tap             h_p[k] = s sinc(t) cos^2(pi t / (2 Z)),  t = clamp(s (k - p / L), -Z, Z),
 *                   sinc(u) = sin(pi u) / (pi u), sinc(0) = 1.  At |t| = Z the window is 0: k = -Wd ... Wd + 1 covers the
 *                   support for every p.
 *   the bank        (L, K) floats, row p = h_p[-Wd ... Wd + 1]: computed by the CALLER in float64, rounded to fp32 once
 *                   (slu_hip/ops.py resample_bank).  The library computes no tap.
 *   output          y[n] = sum_k h_p[k] x[q + k], x = 0 outside [0, len), k ascending, one fp32 accumulator that starts
 *                   at +0 and takes one fmaf per tap (the taps that meet x = 0 included): the result does not depend on
 *                   the tiling, on T_in or on T_out.
 *   tail            y[n] = +0.0f exactly for n_out <= n < T_out.
 *   identity        a row whose bank index is -1 (fi == fo) is copied bit for bit, PCM16 rows as (float)sample * in_scale:
 *                   it is NOT the s = 0.99 filter.  Its n_out is len.
 *   what is read    nothing of a row at or beyond lengths_in[b]: a NaN there reaches no output bit.
 *   determinism     no atomics; the same call twice is bit-equal; row b's result is that of the row converted alone.
 *
 * slu_wave_resample_bank_size(fi, fo): L K, the number of floats of the (fi, fo) bank; 0 when the pair is refused: a rate
 * outside [1000, 384000], or L K > 2^20 (44101 -> 16000 has 576 000 floats and passes, 383999 -> 16000 does not).  fi == fo
 * needs no bank; the answer is then the bank the formulas would give (L = 1), which nothing uses.  Pure host arithmetic.
 *
 * slu_wave_resample arguments (as slu_wave_augment_len's where they coincide):
 *   in          (B, T_in) row-major: fp32, or int16 when in_pcm16 != 0 (then the sample is (float)v * in_scale).
 *   lengths_in  (B) int32: the caller guarantees 1 <= lengths_in[b] <= T_in; the kernel clamps into [0, T_in], so a wrong
 *               value reads nothing out of bounds.
 *   bank_idx    (B) int32: the row's bank, -1 = identity.  An index >= n_banks, or a descriptor that does not fit the
 *               banks (below), gives a row of zeros and lengths_out 0; nothing is indexed out of bounds.
 *   banks       (bank_floats) fp32: the banks one behind the other.
 *   desc        (n_banks, 4) int32: L, M, Wd, offset (in floats) of each bank; it fits when L, M >= 1, Wd >= 1,
 *               offset >= 0 and offset + L (2 Wd + 2) <= bank_floats.  banks and desc may be NULL when n_banks == 0.
 *   out         (B, T_out) fp32, every element written.
 *   lengths_out (B) int32 or NULL: min(n_out, T_out).  The host knows n_out without reading it
 *               (ops.resample_out_lengths) and refuses T_out < n_out.
 * One launch: one workgroup of 256 threads per (row, tile of 1024 output samples); the grid depends on (B, T_out) alone.
 * The tile's source window ((1024 M) / L + K samples) is staged in LDS with coalesced loads, PCM16 converted once, zeros
 * outside [0, len); a window of more than 8192 samples (M / L beyond about 7.9) is read from global memory instead, the
 * same arithmetic in the same order.  The taps are read from the bank through the caches.
 * SLU_ERR_INVALID_ARG: a NULL pointer that may not be NULL, B outside [1, 65535], T_in or T_out outside [1, 2^31 - 1],
 * n_banks outside [0, 65535], bank_floats outside [0, 2^31 - 1], in_scale not finite — the message names the argument.
 * All refusals happen before any launch.
 */
#ifndef SLU_RESAMPLE_H
#define SLU_RESAMPLE_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SLU_RESAMPLE_ABI_VERSION 1

int64_t slu_wave_resample_bank_size(int64_t fi, int64_t fo);
int slu_wave_resample(const void* in, int in_pcm16, float in_scale, int64_t B, int64_t T_in, const int32_t* lengths_in,
                      const int32_t* bank_idx, const float* banks, int64_t bank_floats, const int32_t* desc,
                      int64_t n_banks, float* out, int64_t T_out, int32_t* lengths_out, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* SLU_RESAMPLE_H */
