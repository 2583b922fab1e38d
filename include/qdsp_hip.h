/*
 * qdsp_hip.h -- C ABI of libqdsp_hip.so: qdsp's FIR / polyphase-resampler / NCO-mixer
 * hot path as hand-written HIP kernels for MI355X (gfx950).
 *
 * This is the drop-in boundary.  The reference (AlexandreRouma/qdsp) has no FFI of its
 * own: its blocks call VOLK from inside `run()`.  Each entry point below replaces one of
 * those call sites (cited per function, paths relative to the reference tree), and is
 * what a HIP-backed `dsp::FIR<T>::run()` etc. binds to -- see INTEGRATION.md and the
 * host-side mirror in qdsp_amd/host/dsp/.
 *
 * Conventions
 *   - plain C: pointers, sizes, opaque `void*` handles; no C++/torch types, no exceptions.
 *   - complex samples are interleaved {re, im} float pairs (dsp::complex_t,
 *     src/dsp/types.h:65-66); `count` is always in SAMPLES, not floats.
 *   - return value: 0 (or a non-negative count where stated) on success, negative on
 *     failure: -(hipError_t) for runtime errors, QDSP_HIP_E* below for argument errors.
 *     qdsp_hip_error_string() decodes either.
 *   - every handle is bound to one device and is NOT thread-safe; as in the reference,
 *     `run()` owns it on the block's worker thread and setters are called with the block
 *     stopped (src/dsp/block.h:108-120).
 *   - `*_process`      : host pointers (the stream's readBuf / writeBuf).  Synchronous:
 *                        on return the output is in host memory, so `out.swap()` may
 *                        follow immediately (src/dsp/filter.h:69).
 *   - `*_process_dev`  : device pointers + a hipStream_t (as void*).  Asynchronous on that
 *                        stream; state (history, NCO phase) is advanced in stream order.
 *                        in/out must not alias.  `stream` NULL = HIP's default stream.
 *                        All calls on one handle must be stream-ordered by the caller.
 *   - `*_process_ex`   : like `*_process`, but each side says where its buffer lives
 *                        (`in_on_device` / `out_on_device`): a block whose neighbour is
 *                        another HIP-backed block reads / writes the stream's device-resident
 *                        buffer and skips that PCIe copy.  Synchronous.
 *   - one `process*` call == one `run()` of the reference block: history carries over
 *     exactly as the reference's memmove does, and the resampler's phase counter restarts
 *     at 0 (src/dsp/resampling.h:114,121).
 */
#ifndef QDSP_HIP_H
#define QDSP_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define QDSP_HIP_ABI_VERSION 1

#define QDSP_HIP_EINVAL (-10001)  /* bad argument                                    */
#define QDSP_HIP_ENOMEM (-10002)  /* host allocation failed                          */
#define QDSP_HIP_ESIZE (-10003)   /* count exceeds the handle's max_block            */
#define QDSP_HIP_ENODEV (-10004)  /* no usable gfx950 device / device index invalid  */
#define QDSP_HIP_ERCCL (-10005)   /* RCCL not loadable, or an RCCL call failed (ring)  */

/* ---- library ------------------------------------------------------------------------- */
int qdsp_hip_abi_version(void);
const char* qdsp_hip_error_string(int code);
int qdsp_hip_device_count(int* count);
/* Name / gcnArchName of a device into caller buffers (may be NULL). */
int qdsp_hip_device_info(int device, char* name, int name_len, char* arch, int arch_len,
                         int* compute_units);
/* The QDSP_HIP_* tuning / experiment variables are read ONCE, when the library first needs one, into an
 * immutable table -- no getenv on the call path (the reference blocks hand over <= 1e6 samples per call, src/dsp/stream.h:7:
 * a call lasts 3-8 us).  A process that changes its environment afterwards (tests, tuning scripts) calls this to have the
 * table rebuilt; calls already running keep the table they started with.  Returns 0. */
int qdsp_hip_reload_env(void);

/* Link codes of the *_process_ex / sine generate `*_on_device` arguments (the device-resident companion of
 * dsp::stream<T>, src/dsp/stream.h:21-125): 0 = host buffer; 1 = device buffer, complete on entry / on return;
 * QDSP_HIP_LINK_PIPELINED = device buffer on a pipelined link: the call runs on the library's one in-order stream
 * per device and does not wait for a block it hands to such a link -- the consumer's call runs on the same stream,
 * behind it.  Valid when both ends launch before they swap / flush the stream<T> (the blocks of
 * qdsp_amd/host/dsp do).  A host input is always waited for (its buffer is released on return). */
#define QDSP_HIP_LINK_HOST 0
#define QDSP_HIP_LINK_DEVICE 1
#define QDSP_HIP_LINK_PIPELINED 2
/* host buffer (pinned), completion deferred to the consumer: the call records the handle's done event
 * (qdsp_hip_set_done_event) behind its work and returns; whoever reads the buffer waits for that event first
 * (dsp::stream<T>::read does, the event travels with the buffer through swap()).  Output side only. */
#define QDSP_HIP_LINK_HOST_DEFERRED 3
int qdsp_hip_event_create(int device, void** ev);
int qdsp_hip_event_destroy(void* ev);
int qdsp_hip_event_wait(void* ev);
int qdsp_hip_set_done_event(void* handle, void* ev);   /* any FIR / resampler / mixer / VFO / sine / demodulator handle */

/* ---- memory helpers (for hosts that do not link the HIP runtime themselves) ----------- */
/* Pinned host memory: replaces volk_malloc for stream buffers (src/dsp/stream.h:25-26) so
 * readBuf/writeBuf are DMA-able without staging. */
int qdsp_hip_host_alloc(void** p, size_t bytes);
int qdsp_hip_host_free(void* p);
/* Pin / unpin memory the caller already owns (e.g. an unmodified reference stream). */
int qdsp_hip_host_register(void* p, size_t bytes);
int qdsp_hip_host_unregister(void* p);
int qdsp_hip_dev_alloc(int device, void** p, size_t bytes);
int qdsp_hip_dev_free(int device, void* p);
int qdsp_hip_memcpy_h2d(int device, void* d_dst, const void* h_src, size_t bytes);
int qdsp_hip_memcpy_d2h(int device, void* h_dst, const void* d_src, size_t bytes);
int qdsp_hip_memcpy_d2d(int device, void* d_dst, const void* d_src, size_t bytes);
/* the same for a block that forwards data between links (Splitter, src/dsp/routing.h:47-57): ordered behind a
 * QDSP_HIP_LINK_PIPELINED source, not waited for when the destination link is pipelined as well */
int qdsp_hip_memcpy_d2d_link(int device, void* d_dst, const void* d_src, size_t bytes, int in_link, int out_link);
int qdsp_hip_memcpy_d2h_link(int device, void* h_dst, const void* d_src, size_t bytes, int in_link);
int qdsp_hip_device_sync(int device);

/* ---- FIR<complex_t> : src/dsp/filter.h:51-74 ------------------------------------------ */
/* Replaces the loop of volk_32fc_32f_dot_prod_32fc calls (filter.h:63-67) plus the
 * memcpy-into-history (filter.h:55) and memmove (filter.h:71):
 *     y[n] = sum_{k<ntaps} taps[k] * x[n - (ntaps-1) + k]
 * History = the last ntaps-1 input samples, zero after create/reset (the reference leaves
 * it uninitialised, filter.h:28).  max_block bounds `count` of the host-pointer path only
 * (STREAM_BUFFER_SIZE, src/dsp/stream.h:7). */
int qdsp_hip_fir_cf32_create(void** h, int device, const float* taps, int ntaps, int max_block);
int qdsp_hip_fir_cf32_process(void* h, const float* in_iq, int count, float* out_iq);
int qdsp_hip_fir_cf32_process_dev(void* h, const void* d_in, int64_t count, void* d_out,
                                  void* hip_stream);
int qdsp_hip_fir_cf32_process_ex(void* h, const void* in, int in_on_device, int count, void* out,
                                 int out_on_device);
/* FIR<T>::updateWindow (filter.h:43-49): new taps; history is kept (resized, newest
 * samples preserved) as the reference keeps its buffer. */
int qdsp_hip_fir_cf32_set_taps(void* h, const float* taps, int ntaps);
/* Algorithm choice.  QDSP_HIP_FIR_DIRECT: direct form, taps accumulated in order 0..ntaps-1
 * with one fused multiply-add each (bit-identical to a k-ordered fmaf chain).
 * QDSP_HIP_FIR_FFT: 4096-point overlap-save fast convolution (~135 FLOP/sample instead of
 * 4*ntaps; FP32 FFT rounding, ~3e-7 RMS relative to the direct form).  QDSP_HIP_FIR_AUTO
 * (default): FIR<complex_t> follows a measured table (qdsp_amd/csrc/dispatch_table.inc: call size x taps -> the fastest of the
 * latency direct form, the direct form, the one-wave 1024-point and the 4096-point overlap-save kernels); other data types:
 * FFT for >= 8 taps on calls of >= 65536 samples (it runs at copy speed whatever the
 * taps; measured crossover), direct form otherwise. */
#define QDSP_HIP_FIR_AUTO 0
#define QDSP_HIP_FIR_DIRECT 1
#define QDSP_HIP_FIR_FFT 2
int qdsp_hip_fir_cf32_set_mode(void* h, int mode);
int qdsp_hip_fir_cf32_reset(void* h);
/* History access for the multi-GPU halo: `nsamples` = ntaps-1.
 * get/set copy through host memory; history_dev exposes the device buffer that the NEXT
 * process call will read, so an RCCL recv can land in it directly. */
int qdsp_hip_fir_cf32_history_len(void* h);
int qdsp_hip_fir_cf32_get_history(void* h, float* hist_iq);
int qdsp_hip_fir_cf32_set_history(void* h, const float* hist_iq);
int qdsp_hip_fir_cf32_history_dev(void* h, void** d_hist);
/* Install the `history_len` INPUT samples that precede the next call (device memory, e.g. the
 * buffer an RCCL recv of the neighbour's tail just filled), asynchronously on `hip_stream`.
 * xlate_fir_decim_cf32 keeps its history rotated (as the reference resampler's buffer holds
 * the xlator's output): it rotates the samples itself, with the NCO phases they would have
 * had (set / advance the phase first). */
int qdsp_hip_fir_cf32_set_history_dev(void* h, const void* d_hist, void* hip_stream);
void qdsp_hip_fir_cf32_destroy(void* h);

/* ---- FIR<float> : src/dsp/filter.h:58-62 (volk_32f_x2_dot_prod_32f) -------------------- */
int qdsp_hip_fir_f32_create(void** h, int device, const float* taps, int ntaps, int max_block);
int qdsp_hip_fir_f32_process(void* h, const float* in, int count, float* out);
int qdsp_hip_fir_f32_process_dev(void* h, const void* d_in, int64_t count, void* d_out,
                                 void* hip_stream);
int qdsp_hip_fir_f32_process_ex(void* h, const void* in, int in_on_device, int count, void* out,
                                int out_on_device);
int qdsp_hip_fir_f32_set_taps(void* h, const float* taps, int ntaps);
int qdsp_hip_fir_f32_set_mode(void* h, int mode); /* as for cf32; the overlap-save form carries two real
                                                    * segments per complex transform (auto: >= 96 taps) */
int qdsp_hip_fir_f32_reset(void* h);
int qdsp_hip_fir_f32_history_len(void* h);
int qdsp_hip_fir_f32_get_history(void* h, float* hist);
int qdsp_hip_fir_f32_set_history(void* h, const float* hist);
int qdsp_hip_fir_f32_history_dev(void* h, void** d_hist);
int qdsp_hip_fir_f32_set_history_dev(void* h, const void* d_hist, void* hip_stream);
void qdsp_hip_fir_f32_destroy(void* h);

/* ---- PolyphaseResampler<complex_t> : src/dsp/resampling.h:99-132 ----------------------- */
/* Rational interp/decim resampler; a pure decimator when interp == 1.  `taps` is the
 * prototype exactly as the window hands it over (already scaled by interp,
 * resampling.h:34); the phase split of buildTapPhases (resampling.h:137-166) happens
 * inside.  Replaces the volk_32fc_32f_dot_prod_32fc loop (resampling.h:121-125):
 *     P = ceil(ntaps/interp);  outCount = count*interp/decim;
 *     y[n] = sum_{t<P} phase[(n*decim) % interp][t] * x[(n*decim)/interp - P + t]
 * History = last P input samples (zero after create/reset, resampling.h:39).
 * process* return outCount (>= 0) or a negative error. */
int qdsp_hip_decim_cf32_create(void** h, int device, const float* taps, int ntaps, int interp,
                               int decim, int max_block);
int qdsp_hip_decim_cf32_process(void* h, const float* in_iq, int count, float* out_iq);
int64_t qdsp_hip_decim_cf32_process_dev(void* h, const void* d_in, int64_t count, void* d_out,
                                        void* hip_stream);
int qdsp_hip_decim_cf32_process_ex(void* h, const void* in, int in_on_device, int count, void* out,
                                   int out_on_device);
/* updateWindow / setInSampleRate / setOutSampleRate (resampling.h:53-93) all funnel here. */
int qdsp_hip_decim_cf32_configure(void* h, const float* taps, int ntaps, int interp, int decim);
int64_t qdsp_hip_decim_cf32_out_size(void* h, int64_t count); /* calcOutSize, :95-97 */
/* QDSP_HIP_FIR_AUTO / _DIRECT / _FFT as for the FIR.  The overlap-save path serves interp == 1
 * with any decimation >= 2 (decim in {2, 4, 8, 16}: pruned inverse transform; others: full
 * inverse, every decim-th output stored).  AUTO (measured crossovers): short and medium filters
 * (decim 2..8, 10, 12, 16; up to 150..256 taps) run a strided-window direct kernel; decimations from 9 on with
 * up to ~9 taps per unit of decimation (the VFO's usual shape) the general direct kernel, which streams the
 * input once (4-16 lanes share an output's taps once a tile holds fewer outputs than a workgroup has lanes:
 * partial sums are then added in chunk order, not tap order); longer filters the overlap-save path on calls of
 * >= 65536 samples; the rest a direct form.  QDSP_HIP_FIR_DIRECT always means a direct form (decim <= 8: the
 * de-interleaved, k-ordered kernel; above: the general kernel).  interp > 1 is direct form whatever the mode. */
int qdsp_hip_decim_cf32_set_mode(void* h, int mode);
int qdsp_hip_decim_cf32_reset(void* h);
int qdsp_hip_decim_cf32_history_len(void* h); /* = taps per phase */
int qdsp_hip_decim_cf32_get_history(void* h, float* hist_iq);
int qdsp_hip_decim_cf32_set_history(void* h, const float* hist_iq);
int qdsp_hip_decim_cf32_history_dev(void* h, void** d_hist);
int qdsp_hip_decim_cf32_set_history_dev(void* h, const void* d_hist, void* hip_stream);
void qdsp_hip_decim_cf32_destroy(void* h);

/* ---- PolyphaseResampler<float> : src/dsp/resampling.h:113-119 -------------------------- */
int qdsp_hip_decim_f32_create(void** h, int device, const float* taps, int ntaps, int interp,
                              int decim, int max_block);
int qdsp_hip_decim_f32_process(void* h, const float* in, int count, float* out);
int64_t qdsp_hip_decim_f32_process_dev(void* h, const void* d_in, int64_t count, void* d_out,
                                       void* hip_stream);
int qdsp_hip_decim_f32_process_ex(void* h, const void* in, int in_on_device, int count, void* out,
                                  int out_on_device);
int qdsp_hip_decim_f32_configure(void* h, const float* taps, int ntaps, int interp, int decim);
int64_t qdsp_hip_decim_f32_out_size(void* h, int64_t count);
int qdsp_hip_decim_f32_set_mode(void* h, int mode); /* as for cf32 (interp 1; auto: >= 32 taps per branch) */
int qdsp_hip_decim_f32_reset(void* h);
int qdsp_hip_decim_f32_history_len(void* h);
int qdsp_hip_decim_f32_get_history(void* h, float* hist);
int qdsp_hip_decim_f32_set_history(void* h, const float* hist);
int qdsp_hip_decim_f32_history_dev(void* h, void** d_hist);
int qdsp_hip_decim_f32_set_history_dev(void* h, const void* d_hist, void* hip_stream);
void qdsp_hip_decim_f32_destroy(void* h);

/* ---- FrequencyXlator<complex_t> : src/dsp/processing.h:55-70 --------------------------- */
/* Replaces volk_32fc_s32fc_x2_rotator_32fc (processing.h:64): y[n] = x[n] * phase_n,
 * phase_{n+1} = phase_n * phase_inc, phase_0 = (1,0) after create.  phase_inc is the
 * float pair the reference computes in init/setFrequency (processing.h:20,48).
 * The device NCO is not recursive: phase_n = phase_0 * exp(j*n*arg(phase_inc)) with a
 * 64-bit fixed-point phase accumulator, so it has none of the float phasor's drift
 * (DESIGN.md "NCO").  The carried phase is readable/writable as the reference's
 * lv_32fc_t `phase`. */
int qdsp_hip_xlate_cf32_create(void** h, int device, float phase_inc_re, float phase_inc_im,
                               int max_block);
int qdsp_hip_xlate_cf32_process(void* h, const float* in_iq, int count, float* out_iq);
int qdsp_hip_xlate_cf32_process_dev(void* h, const void* d_in, int64_t count, void* d_out,
                                    void* hip_stream);
int qdsp_hip_xlate_cf32_process_ex(void* h, const void* in, int in_on_device, int count, void* out,
                                   int out_on_device);
int qdsp_hip_xlate_cf32_set_phase_inc(void* h, float phase_inc_re, float phase_inc_im);
int qdsp_hip_xlate_cf32_get_phase(void* h, float* phase_re, float* phase_im);
int qdsp_hip_xlate_cf32_set_phase(void* h, float phase_re, float phase_im);
/* Jump the NCO as if `nsamples` samples had been processed (multi-GPU chunk start,
 * no communication needed for the phase). */
int qdsp_hip_xlate_cf32_advance(void* h, int64_t nsamples);
/* VOLK's rotator renormalises its float phasor only every 512 samples and at the end of a
 * call, so what it multiplies by has magnitude |phase_inc|^(n mod 512) (n from the start of
 * the call; |phase_inc| of the rounded float pair is 1 +- ~3e-8).  on = 1 (default)
 * reproduces that deterministic gain so results sit within float rounding of the
 * reference; on = 0 gives the ideal unit-magnitude NCO. */
int qdsp_hip_xlate_cf32_set_volk_gain(void* h, int on);
void qdsp_hip_xlate_cf32_destroy(void* h);

/* ---- SineSource : src/dsp/source.h:5-71 ------------------------------------------------- */
/* The reference runs volk_32fc_s32fc_x2_rotator_32fc over a buffer of ones (source.h:55-59):
 * out[n] = phase_n, phase_{n+1} = phase_n * phase_inc, phase_0 = (1,0).  Same NCO as
 * xlate_cf32 with no input traffic.  generate(): `out` on the host (synchronous copy) or
 * device-resident (out_on_device = 1); generate_dev(): asynchronous on `hip_stream`. */
int qdsp_hip_sine_cf32_create(void** h, int device, float phase_inc_re, float phase_inc_im, int max_block);
int qdsp_hip_sine_cf32_generate(void* h, int count, void* out, int out_on_device);
int qdsp_hip_sine_cf32_generate_dev(void* h, int64_t count, void* d_out, void* hip_stream);
int qdsp_hip_sine_cf32_set_phase_inc(void* h, float phase_inc_re, float phase_inc_im);
int qdsp_hip_sine_cf32_get_phase(void* h, float* phase_re, float* phase_im);
int qdsp_hip_sine_cf32_set_volk_gain(void* h, int on);
void qdsp_hip_sine_cf32_destroy(void* h);

/* ---- VFO : src/dsp/vfo.h:19-36 (FrequencyXlator -> PolyphaseResampler), fused ---------- */
/* One kernel does what the reference runs as two blocks/threads with a stream hop between
 * them: rotate while staging into LDS, then the polyphase dot products.  Semantics are
 * those of xlate_cf32 followed by decim_cf32 (history holds ROTATED samples, exactly as
 * the reference resampler's buffer does).  Returns outCount or a negative error. */
int qdsp_hip_xlate_fir_decim_cf32_create(void** h, int device, const float* taps, int ntaps,
                                         int interp, int decim, float phase_inc_re,
                                         float phase_inc_im, int max_block);
int qdsp_hip_xlate_fir_decim_cf32_process(void* h, const float* in_iq, int count, float* out_iq);
int64_t qdsp_hip_xlate_fir_decim_cf32_process_dev(void* h, const void* d_in, int64_t count,
                                                  void* d_out, void* hip_stream);
int qdsp_hip_xlate_fir_decim_cf32_process_ex(void* h, const void* in, int in_on_device, int count,
                                             void* out, int out_on_device);
int qdsp_hip_xlate_fir_decim_cf32_configure(void* h, const float* taps, int ntaps, int interp,
                                            int decim);
int qdsp_hip_xlate_fir_decim_cf32_set_phase_inc(void* h, float phase_inc_re, float phase_inc_im);
int qdsp_hip_xlate_fir_decim_cf32_get_phase(void* h, float* phase_re, float* phase_im);
int qdsp_hip_xlate_fir_decim_cf32_set_phase(void* h, float phase_re, float phase_im);
int qdsp_hip_xlate_fir_decim_cf32_advance(void* h, int64_t nsamples);
int qdsp_hip_xlate_fir_decim_cf32_set_volk_gain(void* h, int on);
int64_t qdsp_hip_xlate_fir_decim_cf32_out_size(void* h, int64_t count);
int qdsp_hip_xlate_fir_decim_cf32_set_mode(void* h, int mode);
int qdsp_hip_xlate_fir_decim_cf32_reset(void* h);
int qdsp_hip_xlate_fir_decim_cf32_history_len(void* h);
int qdsp_hip_xlate_fir_decim_cf32_get_history(void* h, float* hist_iq);
int qdsp_hip_xlate_fir_decim_cf32_set_history(void* h, const float* hist_iq);
int qdsp_hip_xlate_fir_decim_cf32_history_dev(void* h, void** d_hist);
int qdsp_hip_xlate_fir_decim_cf32_set_history_dev(void* h, const void* d_hist, void* hip_stream);
void qdsp_hip_xlate_fir_decim_cf32_destroy(void* h);

/* ---- channelizer: Splitter -> N x VFO (src/dsp/routing.h:47-57 + src/dsp/vfo.h), batched ---- */
/* N frequency-translating decimators on ONE input stream: channel c is exactly
 * xlate_fir_decim_cf32 with phase increment (phase_inc_re[c], phase_inc_im[c]); all channels
 * share taps / interp / decim.  Output is channel-major: channel c's samples start at
 * out + c*out_stride (complex samples).  process* return the per-channel output count.
 * 64 channels spaced 1/64 turn per sample with decim 64 and <= 256 taps run as ONE polyphase
 * filter-bank kernel (qdsp_amd/csrc/chan.hip); any other plan runs one fused kernel per
 * channel on the same stream.  set_mode(QDSP_HIP_FIR_DIRECT) forces the per-channel form. */
int qdsp_hip_chan_cf32_create(void** h, int device, const float* taps, int ntaps, int interp,
                              int decim, int nchan, const float* phase_inc_re,
                              const float* phase_inc_im, int max_block);
int qdsp_hip_chan_cf32_process(void* h, const float* in_iq, int count, float* out_iq, int out_stride);
int64_t qdsp_hip_chan_cf32_process_dev(void* h, const void* d_in, int64_t count, void* d_out,
                                       int64_t out_stride, void* hip_stream);
/* The same operator inside a block graph (Splitter -> N x VFO with identical filters, src/dsp/routing.h:47-57): ONE batched
 * launch, channel c's samples into its own stream buffer outs[c] with link code out_links[c] (QDSP_HIP_LINK_HOST_DEFERRED:
 * pinned host buffer, stored by the kernel itself, complete once `done_event` has fired -- or QDSP_HIP_LINK_HOST: complete on
 * return; QDSP_HIP_LINK_DEVICE / _PIPELINED as for *_process_ex).  Always the per-channel (non-uniform) form.  Returns the
 * per-channel output count; QDSP_HIP_ESIZE / _EINVAL when a buffer cannot be served this way (pageable or > 1 MiB host
 * output, taps beyond LDS): the caller then runs the channels one by one. */
int64_t qdsp_hip_chan_cf32_process_links(void* h, const void* in, int in_link, int count, void* const* outs, const int* out_links,
                                         void* done_event);
/* NCO phase (exact) and filter history of channel `chan` into (to_vfo != 0) or out of (to_vfo == 0) a stand-alone
 * xlate_fir_decim_cf32 handle of the same design: how a Splitter hands running VFOs to a bank and back without a glitch.
 * Synchronises the device; histories of different length are zeroed instead of copied. */
int qdsp_hip_chan_cf32_move_channel_state(void* h, int chan, void* vfo_handle, int to_vfo);
int64_t qdsp_hip_chan_cf32_out_size(void* h, int64_t count);
int qdsp_hip_chan_cf32_set_phase_inc(void* h, int chan, float phase_inc_re, float phase_inc_im);
int qdsp_hip_chan_cf32_set_mode(void* h, int mode);
int qdsp_hip_chan_cf32_set_volk_gain(void* h, int on);
int qdsp_hip_chan_cf32_reset(void* h);
/* Time-sharding a stream over GPUs (as for xlate_fir_decim_cf32): history_len raw INPUT
 * samples that precede the next call, rotated internally with each channel's NCO; advance
 * moves every channel's NCO by n samples without processing. */
int qdsp_hip_chan_cf32_history_len(void* h);
int qdsp_hip_chan_cf32_set_history_dev(void* h, const void* d_hist, void* hip_stream);
int qdsp_hip_chan_cf32_advance(void* h, int64_t n);
int qdsp_hip_chan_cf32_channels(void* h);
void qdsp_hip_chan_cf32_destroy(void* h);

/* ---- element-wise two-input blocks: Add / Substract / Multiply (src/dsp/math.h:7-145) ---- */
/* out[i] = a[i] op b[i] over `count` samples; complex_data: samples are interleaved {re, im}
 * pairs and QDSP_HIP_MATH_MUL is the complex product (volk_32fc_x2_multiply_32fc, math.h:127),
 * add / subtract are per float (math.h:33,80).  Results are bit-identical to VOLK's generic
 * kernels (separately rounded products and sums).  Stateless apart from staging buffers.
 * process: host pointers, synchronous; process_ex: each side host or device (1 = device);
 * process_dev: asynchronous on hip_stream, pointers 16-byte aligned. */
#define QDSP_HIP_MATH_ADD 0
#define QDSP_HIP_MATH_SUB 1
#define QDSP_HIP_MATH_MUL 2
int qdsp_hip_math_create(void** h, int device, int op, int complex_data, int max_block);
int qdsp_hip_math_process(void* h, const void* a, const void* b, int count, void* out);
int qdsp_hip_math_process_ex(void* h, const void* a, int a_dev, const void* b, int b_dev, int count,
                             void* out, int out_dev);
int qdsp_hip_math_process_dev(void* h, const void* d_a, const void* d_b, int64_t count, void* d_out,
                              void* hip_stream);
void qdsp_hip_math_destroy(void* h);

/* ---- demodulators : src/dsp/demodulator.h ------------------------------------------------ */
/* The data-parallel ones; what follows a VFO or a channelizer channel.  Output per input sample: one float (FM, AM), or a
 * stereo_t {l, r} with l == r (FM_STEREO).
 *   FM   cp[i] = fast_arctan2(im, re) (demodulator.h:14-30); d = cp[i] - cp[i-1], wrapped once by +-2 pi (with the float
 *        literal 3.1415926535f); out = d / phasorSpeed, phasorSpeed = (2 * FL_M_PI) / (sampleRate / deviation) in float.
 *        cp[-1] is the last phase of the previous call, 0 after create / reset; it stays on the device (no call waits for
 *        it).  Bit-identical to the reference loop (demodulator.h:86-95), call boundaries included.
 *   AM   out = |x| - avg (demodulator.h:353-372), |x| = sqrtf(re*re + im*im) bit-identical to VOLK's generic magnitude;
 *        avg = the mean of THIS call's |x| (per channel), summed in FP64 in a fixed order and rounded once to float: within
 *        an ulp of the exact mean, where the reference's float accumulator may be off by more.
 * nchan channels are processed by one launch: channel-major rows, `in_stride` / `out_stride` samples apart (the layout
 * qdsp_hip_chan_cf32_process_dev writes), each with its own carried phase and phasorSpeed.  process / process_ex (nchan 1):
 * host pointers / link codes as for every *_process_ex, `count` <= max_block where a side is on the host (else
 * QDSP_HIP_ESIZE).  process_dev: the nchan rows back to back (strides = count).  Device pointers: input 8-byte, output
 * 4-byte (FM_STEREO: 8-byte) aligned; 16-byte aligned rows take the vector loads.  set_fm before the first call (default:
 * sample_rate = deviation = 1); `chan` -1 = every channel.  get_phase synchronises the device. */
#define QDSP_HIP_DEMOD_FM 0          /* FloatFMDemod :33-108 */
#define QDSP_HIP_DEMOD_FM_STEREO 1   /* FMDemod :110-187     */
#define QDSP_HIP_DEMOD_AM 2          /* AMDemod :332-378     */
int qdsp_hip_demod_create(void** h, int device, int kind, int nchan, int max_block);
int qdsp_hip_demod_set_fm(void* h, int chan, float sample_rate, float deviation);
int qdsp_hip_demod_process(void* h, const float* in_iq, int count, void* out);
int qdsp_hip_demod_process_ex(void* h, const void* in, int in_link, int count, void* out, int out_link);
int qdsp_hip_demod_process_dev(void* h, const void* d_in, int64_t count, void* d_out, void* hip_stream);
int qdsp_hip_demod_process_batch_dev(void* h, const void* d_in, int64_t count, int64_t in_stride, void* d_out,
                                     int64_t out_stride, void* hip_stream);
int qdsp_hip_demod_get_phase(void* h, int chan, float* phase);
int qdsp_hip_demod_set_phase(void* h, int chan, float phase);
int qdsp_hip_demod_reset(void* h);
void qdsp_hip_demod_destroy(void* h);
/* SSBDemod :380-497: xlate_cf32's NCO (the same 64-bit phase and VOLK gain emulation, so the same deviation from the
 * recursive phasor), only the real part stored.  phase_inc = (cos, sin)(+-(bandWidth / sampleRate) * FL_M_PI) for USB / LSB,
 * (1, 0) for DSB, as SSBDemod::init computes it.  One channel; the entry points are those of xlate_cf32. */
int qdsp_hip_ssb_cf32_create(void** h, int device, float phase_inc_re, float phase_inc_im, int max_block);
int qdsp_hip_ssb_cf32_process(void* h, const float* in_iq, int count, float* out);
int qdsp_hip_ssb_cf32_process_dev(void* h, const void* d_in, int64_t count, void* d_out, void* hip_stream);
int qdsp_hip_ssb_cf32_process_ex(void* h, const void* in, int in_link, int count, void* out, int out_link);
int qdsp_hip_ssb_cf32_set_phase_inc(void* h, float phase_inc_re, float phase_inc_im);
int qdsp_hip_ssb_cf32_get_phase(void* h, float* phase_re, float* phase_im);
int qdsp_hip_ssb_cf32_set_phase(void* h, float phase_re, float phase_im);
int qdsp_hip_ssb_cf32_advance(void* h, int64_t nsamples);
int qdsp_hip_ssb_cf32_set_volk_gain(void* h, int on);
void qdsp_hip_ssb_cf32_destroy(void* h);

/* ---- de-emphasis : BFMDeemp, src/dsp/filter.h:90-173 -------------------------------------- */
/* y[i] = alpha x[i] + (1 - alpha) y[i-1], alpha = dt / (tau + dt), dt = 1.0f / sampleRate, all coefficients in float as the
 * reference computes them.  The recurrence is evaluated as a parallel prefix scan of affine maps composed in FP64, every
 * output rounded to float once: not the bits of the reference's float loop (no reassociated scan can give those), but within
 * 0.5 ulp + 2^-40 * (the same filter run over |x|) of the exact recurrence, and no further from it than the float loop is.
 * Rows are float (MONO) or stereo_t {l, r} (STEREO; l and r filtered independently with the same alpha): nchan channel-major
 * rows, strides in samples, the layout qdsp_hip_demod_process_batch_dev writes; each channel has its own alpha and state.
 * State: y[-1] of the next call, kept on the device in FP64 per channel and component; 0 after create / reset.  get_state
 * rounds it to float (= the last output) and synchronises the device; set_state widens a float.  At the start of a call a
 * state that is not finite reads as 0.  For NaN that is the reference's rule (filter.h:140-145): a NaN input poisons its
 * own component from that sample to the end of the call, the next call starts clean.  For +-Inf it is a deliberate departure:
 * the reference's state would stay Inf for ever; here the outputs from an Inf input to the end of that call are not finite
 * (Inf or NaN, unspecified) and the next call starts from 0.
 * set_bypass(1): process* copies input to output and leaves the state alone (BFMDeemp::bypass).  set before the first call
 * (default: sample_rate 1, tau 0, i.e. alpha 1, y = x); `chan` -1 = every channel.  count == 0 is a no-op.
 * process / process_ex (nchan 1): host pointers / link codes as for every *_process_ex, `count` <= max_block where a side is
 * on the host (else QDSP_HIP_ESIZE).  process_dev: the nchan rows back to back (strides = count).  Device pointers: 4-byte
 * (STEREO: 8-byte) aligned; 16-byte aligned rows take the vector loads and stores.  In place (d_out == d_in, with
 * out_stride == in_stride) is supported and gives the same bits; any other overlap of input and output is not. */
#define QDSP_HIP_DEEMP_MONO   0   /* float rows    */
#define QDSP_HIP_DEEMP_STEREO 1   /* stereo_t rows */
int qdsp_hip_deemp_create(void** h, int device, int kind, int nchan, int max_block);
int qdsp_hip_deemp_set(void* h, int chan, float sample_rate, float tau);
int qdsp_hip_deemp_set_bypass(void* h, int on);
int qdsp_hip_deemp_process(void* h, const float* in, int count, float* out);
int qdsp_hip_deemp_process_ex(void* h, const void* in, int in_link, int count, void* out, int out_link);
int qdsp_hip_deemp_process_dev(void* h, const void* d_in, int64_t count, void* d_out, void* hip_stream);
int qdsp_hip_deemp_process_batch_dev(void* h, const void* d_in, int64_t count, int64_t in_stride, void* d_out,
                                     int64_t out_stride, void* hip_stream);
int qdsp_hip_deemp_get_state(void* h, int chan, float* l, float* r);   /* MONO: r may be NULL */
int qdsp_hip_deemp_set_state(void* h, int chan, float l, float r);
int qdsp_hip_deemp_get_alpha(void* h, int chan, float* alpha);
int qdsp_hip_deemp_reset(void* h);
void qdsp_hip_deemp_destroy(void* h);

/* ---- level blocks : Squelch and AGC, src/dsp/processing.h:424-489 and :83-145 ------------- */
/* Both take one reduction over a call (one run() of the reference) and one pass over it; nchan channel-major rows per launch,
 * strides in samples, each channel with its own level / fall rate and its own state.  Rows of at most 4 tiles of 2048 samples
 * (QDSP_HIP_LEVEL_ROW_TILES lowers that) take one launch that reads the row once (level_row_kernel); longer rows take two
 * (level_partial_kernel, level_apply_kernel).  The state lives on the device; no call waits for it.  count == 0 is a no-op.
 *   Squelch  complex rows in, complex rows out.  mean = the mean of |x| over the call, |x| = sqrtf(re*re + im*im) as VOLK's
 *        generic magnitude, summed in FP64 in a fixed order and rounded once to float (the AM demodulator's rule: the order of
 *        VOLK's float accumulator depends on the host's SIMD width).  The row is open when 10.0f * log10f(mean) >= level[chan],
 *        evaluated on the device: an open row is a bit copy of the input, NaNs included; a closed row is +0.0f in every float.
 *        A mean of 0 gives -inf: closed.  A NaN anywhere in the row makes the mean NaN, the comparison false and the row
 *        closed, as in the reference.  level: -50.0f after create (processing.h:486).  get_open: the decision of the last
 *        call, 0 after create / reset; it synchronises the device.
 *   AGC  float rows in, float rows out.  level is 0 after create / reset.  Each call, on the device:
 *          level = (float)pow(10.0, (double)(((10.0f * log10f(level)) - (cfr * (float)count)) / 10.0f))
 *        with the inner expression in float and cfr = fall_rate / sample_rate in float (processing.h:93,123); then
 *        level = max(level, max_i x[i]) under the reference's `x > level` (signed input as it is, no fabsf; a NaN never wins);
 *        then out[i] = x[i] * (1.0f / level), one rounded reciprocal and one rounded product (volk_32f_s32f_multiply_32f).
 *        Outputs and level are bit-identical to the reference loop wherever the call's maximum sets the level; where the
 *        decayed level stands, it carries the device's log10f and pow (tests/test_level_cpu.py: agc_decay_bound).
 *        The reference's corner cases are kept:  a level of 0 with no positive sample gives out = x * inf (+-inf, NaN for 0);
 *        an Inf input pins the level at Inf (outputs 0, NaN at the Inf) until reset or set_level;  a NaN input yields a NaN
 *        output at that sample only and leaves the level alone.
 *        set(chan, fall_rate, sample_rate): default fall_rate 0, sample_rate 1; a sample_rate that is not finite and positive
 *        or a fall_rate that is not finite is QDSP_HIP_EINVAL.  get_level synchronises the device.
 * `chan` -1 = every channel (set_level, set).  process / process_ex (nchan 1): host pointers / link codes as for every
 * *_process_ex, `count` <= max_block where a side is on the host (else QDSP_HIP_ESIZE).  process_dev: the nchan rows back to
 * back (strides = count).  Device pointers: Squelch 8-byte, AGC 4-byte aligned; 16-byte aligned rows whose strides are whole
 * 16-byte units take the vector loads and stores.  In place (d_out == d_in with out_stride == in_stride) is supported in both
 * forms and gives the same bits; any other overlap of the spans of input and output is QDSP_HIP_EINVAL. */
int qdsp_hip_squelch_create(void** h, int device, int nchan, int max_block);
int qdsp_hip_squelch_set_level(void* h, int chan, float level_db);
int qdsp_hip_squelch_get_open(void* h, int chan, int* open);
int qdsp_hip_squelch_process(void* h, const float* in_iq, int count, float* out_iq);
int qdsp_hip_squelch_process_ex(void* h, const void* in, int in_link, int count, void* out, int out_link);
int qdsp_hip_squelch_process_dev(void* h, const void* d_in, int64_t count, void* d_out, void* hip_stream);
int qdsp_hip_squelch_process_batch_dev(void* h, const void* d_in, int64_t count, int64_t in_stride, void* d_out,
                                       int64_t out_stride, void* hip_stream);
int qdsp_hip_squelch_reset(void* h);
void qdsp_hip_squelch_destroy(void* h);
int qdsp_hip_agc_create(void** h, int device, int nchan, int max_block);
int qdsp_hip_agc_set(void* h, int chan, float fall_rate, float sample_rate);
int qdsp_hip_agc_get_level(void* h, int chan, float* level);
int qdsp_hip_agc_set_level(void* h, int chan, float level);
int qdsp_hip_agc_process(void* h, const float* in, int count, float* out);
int qdsp_hip_agc_process_ex(void* h, const void* in, int in_link, int count, void* out, int out_link);
int qdsp_hip_agc_process_dev(void* h, const void* d_in, int64_t count, void* d_out, void* hip_stream);
int qdsp_hip_agc_process_batch_dev(void* h, const void* d_in, int64_t count, int64_t in_stride, void* d_out,
                                   int64_t out_stride, void* hip_stream);
int qdsp_hip_agc_reset(void* h);
void qdsp_hip_agc_destroy(void* h);

/* ---- feed-forward AGC : FeedForwardAGC<T>, src/dsp/processing.h:147-233 --------------------- */
/* A sliding-window peak normaliser with no recurrence; nchan channel-major rows per call, strides in samples.  With the stream of
 * all samples ever handed to a row, x[0], x[1], ..., and the window W (`window`, 1 .. 4096; the reference has 1024):
 *   y[p] = x[p] / level[p],   level[p] = max(1e-4f, max over j in [0, W) of a(x[p + j]))
 *   QDSP_HIP_FFAGC_REAL     float rows:     a(v) = fabsf(v), y = v / level
 *   QDSP_HIP_FFAGC_COMPLEX  complex_t rows: a(v) = r + 0.4f * r with r = fabsf(v.re), product and sum each rounded to float --
 *        the reference's fastAmplitude (types.h:58-63) takes both of its magnitudes from re, and that is kept: im never enters
 *        the level.  y = {re / level, im / level}, two IEEE divisions.
 * The maximum runs under the reference's `val > level` from 1e-4f: a NaN never wins (it is a NaN output at its own index only);
 * +Inf wins and makes the W outputs whose window holds it 0 (NaN at the Inf itself).  Bit-identical to the reference loop.
 * y[p] needs x[p + W - 1]: the block lags by W - 1 samples.  The handle keeps the last `fill` <= W - 1 inputs not yet output
 * (every row the same number), on the device, double-buffered.  A call of `count` inputs per row emits
 * out = max(0, fill + count - (W - 1)) outputs per row -- the next `out` stream positions -- and leaves fill + count - out; a call
 * that emits nothing still takes its inputs.  The outputs depend on the stream alone, not on where the calls cut it.
 * process / process_ex (nchan 1; link codes as for every *_process_ex; `count` <= max_block where a side is on the host, else
 * QDSP_HIP_ESIZE) and the *_dev entry points return the number of outputs per row (>= 0) or an error.  process_dev: the nchan
 * input rows `count` apart, the output rows out_size(count) apart.  process_batch_dev: in_stride >= count, out_stride >= out.
 * Pointers: 4-byte (REAL) / 8-byte (COMPLEX) aligned; 16-byte aligned output rows whose stride is a whole number of 16-byte units
 * take 16-byte stores, any others narrower ones, with the same bits.  Input and output may not overlap: any overlap of the two row
 * spans is QDSP_HIP_EINVAL (an output depends on the inputs after its own).
 * out_size: what the next call of `count` would emit.  get_history: the `fill` samples held for `chan`, oldest first (`hist` holds
 * window - 1 samples).  set_history: `fill` samples for row `chan` (-1: the same for every row) and the handle's fill; set every
 * row when the fill changes.  get_history / set_history / reset synchronise the device; reset empties the history. */
#define QDSP_HIP_FFAGC_REAL 0
#define QDSP_HIP_FFAGC_COMPLEX 1
int qdsp_hip_ffagc_create(void** h, int device, int kind, int nchan, int max_block, int window);
int qdsp_hip_ffagc_process(void* h, const float* in, int count, float* out);
int qdsp_hip_ffagc_process_ex(void* h, const void* in, int in_link, int count, void* out, int out_link);
int64_t qdsp_hip_ffagc_process_dev(void* h, const void* d_in, int64_t count, void* d_out, void* hip_stream);
int64_t qdsp_hip_ffagc_process_batch_dev(void* h, const void* d_in, int64_t count, int64_t in_stride, void* d_out,
                                         int64_t out_stride, void* hip_stream);
int64_t qdsp_hip_ffagc_out_size(void* h, int64_t count);
int qdsp_hip_ffagc_window(void* h);
int qdsp_hip_ffagc_fill(void* h);
int qdsp_hip_ffagc_get_history(void* h, int chan, float* hist);
int qdsp_hip_ffagc_set_history(void* h, int chan, const float* hist, int fill);
int qdsp_hip_ffagc_reset(void* h);
void qdsp_hip_ffagc_destroy(void* h);

/* ---- complex AGC : ComplexAGC, src/dsp/processing.h:235-298 ---------------------------------- */
/* The per-sample feedback AGC on complex_t rows; nchan channel-major rows per call, strides in samples, each channel with its own
 * set point, maximum gain, rate and gain (FP64, on the device, 1 at creation):
 *   out[i] = in[i] * g;   g += (set_point - |out[i]|) * rate;   if (g > max_gain) g = max_gain
 * While g >= 0 a sample is the map g -> min(a g + b, c), a = 1 - rate |in[i]|, b = set_point rate, c = max_gain, and these maps
 * compose associatively: a row is run as an FP64 prefix scan and every output is rounded to float once.  The result is the
 * exact recurrence of the float parameters to within |y - x g| <= 0.5 ulp(x g) + |x| 2^-40 max(1, g_0 .. g_i) per component and
 * 2^-40 max(1, g_0 .. g_i) on the gain -- closer to it than the reference's float loop is, and therefore not that loop's bits.
 * The scan holds for a row and call if the carried gain is finite and >= 0, 0 <= set_point * rate < inf, max_gain >= 0,
 * rate >= 0, and every sample is finite with rate * |in[i]| <= 1.  This is decided on the device, per row and call, without the
 * host waiting.  A row that fails is run by the reference's loop in float instead, serially by one wave (slow: INTEGRATION.md),
 * from (float) of its gain: outputs and gain are then the float loop's bit for bit, NaN, Inf and negative gains included, and a
 * NaN gain stays NaN until set_gain / reset, as in the reference.  The other rows of the call are not affected.
 * set: chan -1 = every channel; takes effect from the next call; NaN parameters are QDSP_HIP_EINVAL.  set_gain: chan -1 = every
 * channel, any value.  set / get_gain / set_gain / reset synchronise the device; reset puts every gain back to 1.
 * process / process_ex (nchan 1; link codes as for every *_process_ex; `count` <= max_block where a side is on the host, else
 * QDSP_HIP_ESIZE).  process_dev: the nchan rows back to back (strides = count).  Device pointers: 8-byte aligned; 16-byte
 * aligned rows with even strides take the vector loads and stores.  In place (d_out == d_in, with out_stride == in_stride) is
 * supported and gives the same bits, for both kinds of row; any other overlap of input and output is not. */
int qdsp_hip_cagc_create(void** h, int device, int nchan, int max_block);
int qdsp_hip_cagc_set(void* h, int chan, float set_point, float max_gain, float rate);
int qdsp_hip_cagc_get_gain(void* h, int chan, double* gain);
int qdsp_hip_cagc_set_gain(void* h, int chan, double gain);
int qdsp_hip_cagc_process(void* h, const float* in, int count, float* out);
int qdsp_hip_cagc_process_ex(void* h, const void* in, int in_link, int count, void* out, int out_link);
int qdsp_hip_cagc_process_dev(void* h, const void* d_in, int64_t count, void* d_out, void* hip_stream);
int qdsp_hip_cagc_process_batch_dev(void* h, const void* d_in, int64_t count, int64_t in_stride, void* d_out,
                                    int64_t out_stride, void* hip_stream);
int qdsp_hip_cagc_reset(void* h);
void qdsp_hip_cagc_destroy(void* h);

/* ---- Costas loop : CostasLoop<ORDER>, src/dsp/pll.h:47-102 ------------------------------------ */
/* The carrier-recovery loop of PSKDemod on complex_t rows; nchan channel-major rows per call, strides in samples, one order (2, 4
 * or 8) per handle, each channel with its own loop bandwidth, frequency and phase (FP64, on the device, both 0 at creation):
 *   out[i] = vco * in[i];  e = the order's phase error of out[i], clamped to +-1;  freq = clamp(freq + beta e, +-1);
 *   phase += freq + alpha e, wrapped into [-T, T], T = the reference's float 2 pi;  vco = (cos(-phase), sin(-phase))
 * A row is serial; the rows are independent and run one per lane, 16 to a wave.  alpha and beta are the reference's floats (its
 * formula, evaluated on the host); everything else is FP64 and every output is rounded to float once, so the outputs follow the
 * exact recurrence more closely than the reference's float loop does and are not that loop's bits.  Outputs and state do not
 * depend, bit for bit, on how a stream is cut into calls, on the row's place in the batch, on strides, alignment, in-place use
 * or the entry point.
 * Departures from the reference: (1) set_bandwidth takes a finite bandwidth >= 0 whose alpha and beta are finite, anything else is
 * QDSP_HIP_EINVAL: then |freq + alpha e| < 2 pi and the phase is wrapped by one conditional step each way where the reference
 * loops (for ever, on an infinite phase).  (2) A NaN sample makes its row's outputs NaN from that sample to the end of the call,
 * as in the reference, and leaves the row's state NaN; a carried frequency or phase that is not finite reads as 0 at the next
 * call, where the reference stays NaN for ever.  Other rows are not affected.
 * create: the bandwidth is the reference's default 1.0 until set.  set_bandwidth / set_state: chan -1 = every channel; they act
 * from the next call.  set_state: a finite phase beyond +-T is QDSP_HIP_EINVAL.  set_bandwidth / get_state / set_state / reset
 * synchronise the device; reset puts every frequency and phase back to 0.  get_gains: the alpha and beta in use.
 * process / process_ex (nchan 1; link codes as for every *_process_ex; `count` <= max_block where a side is on the host, else
 * QDSP_HIP_ESIZE).  process_dev: the nchan rows back to back (strides = count).  Device pointers: 8-byte aligned.  In place
 * (d_out == d_in, with out_stride == in_stride) is supported and gives the same bits; any other overlap is not.  count 0 launches
 * nothing and keeps the state. */
int qdsp_hip_costas_create(void** h, int device, int order, int nchan, int max_block);
int qdsp_hip_costas_set_bandwidth(void* h, int chan, float bandwidth);
int qdsp_hip_costas_get_gains(void* h, int chan, float* alpha, float* beta);
int qdsp_hip_costas_get_state(void* h, int chan, double* freq, double* phase);
int qdsp_hip_costas_set_state(void* h, int chan, double freq, double phase);
int qdsp_hip_costas_process(void* h, const float* in, int count, float* out);
int qdsp_hip_costas_process_ex(void* h, const void* in, int in_link, int count, void* out, int out_link);
int qdsp_hip_costas_process_dev(void* h, const void* d_in, int64_t count, void* d_out, void* hip_stream);
int qdsp_hip_costas_process_batch_dev(void* h, const void* d_in, int64_t count, int64_t in_stride, void* d_out,
                                      int64_t out_stride, void* hip_stream);
int qdsp_hip_costas_reset(void* h);
void qdsp_hip_costas_destroy(void* h);

/* ---- symbol timing : MMClockRecovery<float | complex_t>, src/dsp/clock_recovery.h:68-243 ------ */
/* The Mueller & Mueller clock recovery of PSKDemod (complex_t rows) and MSKDemod (float rows); kind 0 = float, 1 = complex_t;
 * nchan channel-major rows per call, strides in samples, each channel with its own omega, gains, limit and state, all on the
 * device.  Per row the symbols are a function of the concatenated input, whatever the call cuts.  With x[p] the row's samples
 * numbered from the last reset (x[p] = 0 for p < 0), mu = 0.5, dynOmega = omega and pos = 0 at the start, while pos lies inside
 * the samples received so far:
 *   idx = (int)roundf(mu * 128.0f);  y = sum_{k = 0..7} x[pos - 7 + k] taps[idx][k]: every product in FP64 (exact), added in tap
 *        order in FP64, rounded to float once; per component for complex rows.  y is the next symbol of the row.
 *   e = the phase error of the row's type (clock_recovery.h:152-153 / :157-176), in float, every operation rounded on its own;
 *        clamped to +-1.
 *   dynOmega = clamp(dynOmega + gainOmega e, omegaMin, omegaMax);  mu += dynOmega + muGain e;  pos += floorf(mu);  mu -= floorf(mu).
 * The reference leaves the order of the eight-term sum to VOLK; here it is fixed as stated, so outputs, counts and state do not
 * depend, bit for bit, on the call cuts, the row's place in the batch, strides, alignment or the entry point.
 * The table: 129 rows of 8 taps, the MMSE interpolator for a band of +-0.25 cycles per sample, computed by the library: row m
 * (mu = m / 128) solves R h = p, R[k][l] = sinc((k - l) / 2), p[k] = sinc((3 + mu - k) / 2), sinc(x) = sin(pi x) / (pi x), in
 * FP64; an entry below 1e-9 in magnitude is 0, every other is rounded to six significant decimal digits and then to float
 * (get_interp_taps).  It agrees with the reference's table to 5e-7; set_interp_taps loads any finite table instead, the
 * reference's own for instance, for all channels of the handle.
 * Parameter rule (create, set_omega, set_gains, set_limit; else QDSP_HIP_EINVAL): all values finite, omega > 0, 0 <= rel_limit < 1,
 * and with omegaMin = omega - omega rel_limit, omegaMax = omega + omega rel_limit in float: omegaMin - |mu_gain| >= 1 (every step
 * is at least one sample) and omegaMax + |mu_gain| < 2^20.  Hence a call of `count` samples emits at most
 * out_size(count) = ceil(count / floor(min over channels of (omegaMin - |mu_gain|))) <= count symbols per row.
 * Departures from the reference: its cap of 2 omega count outputs per call cannot bind under the rule and is absent; the delay
 * line is zero after create / reset (the reference's is uninitialised); any count >= 0 is served (the reference copies out of
 * range below 7); its clamp of a negative position is unreachable; set_omega forms the limits from the new omega (the reference's
 * setOmega from the old one) and, like it, restarts dynOmega at omega.  A NaN phase error: the symbol just formed is written, then
 * the row stops -- it emits nothing further and its mu reads back NaN -- until reset or set_state; other rows are not affected.
 * set_* / get_state / set_state / reset / set_interp_taps synchronise the device and act from the next call; chan -1 = every
 * channel.  get_state: mu, dynOmega and next = pos - samples received (>= 0).  set_state: 0 <= mu < 1, dynOmega finite,
 * 0 <= next <= 2^21; detector and delay line are kept.
 * process_batch_dev: asynchronous; out_stride >= out_size(count); d_in != d_out, spans may not overlap; device pointers aligned
 * to the sample (4 / 8 bytes); a row's symbols go to its first slots, the per-row counts to d_counts (int32[nchan], may be NULL)
 * and to the handle (get_counts: the last call's, synchronising).  process_dev: the rows back to back (strides count and
 * out_size(count)).  process / process_ex (nchan 1) return the symbol count; link codes as for every *_process_ex, but the
 * output link is QDSP_HIP_LINK_HOST or _DEVICE only (the count must be known on return: anything else is QDSP_HIP_EINVAL);
 * `count` <= max_block where a side is on the host (else QDSP_HIP_ESIZE). */
int qdsp_hip_mmcr_create(void** h, int device, int kind, int nchan, int max_block, float omega, float gain_omega, float mu_gain,
                         float rel_limit);
int qdsp_hip_mmcr_set_omega(void* h, int chan, float omega);
int qdsp_hip_mmcr_set_gains(void* h, int chan, float gain_omega, float mu_gain);
int qdsp_hip_mmcr_set_limit(void* h, int chan, float rel_limit);
int qdsp_hip_mmcr_get_state(void* h, int chan, float* mu, float* dyn_omega, int* next);
int qdsp_hip_mmcr_set_state(void* h, int chan, float mu, float dyn_omega, int next);
int64_t qdsp_hip_mmcr_out_size(void* h, int64_t count);
int qdsp_hip_mmcr_get_interp_taps(void* h, float* taps);
int qdsp_hip_mmcr_set_interp_taps(void* h, const float* taps);
int qdsp_hip_mmcr_process(void* h, const float* in, int count, float* out);
int qdsp_hip_mmcr_process_ex(void* h, const void* in, int in_link, int count, void* out, int out_link);
int qdsp_hip_mmcr_process_dev(void* h, const void* d_in, int64_t count, void* d_out, void* hip_stream);
int qdsp_hip_mmcr_process_batch_dev(void* h, const void* d_in, int64_t count, int64_t in_stride, void* d_out, int64_t out_stride,
                                    int* d_counts, void* hip_stream);
int qdsp_hip_mmcr_get_counts(void* h, int* counts);
int qdsp_hip_mmcr_reset(void* h);
void qdsp_hip_mmcr_destroy(void* h);

/* ---- FIR over channel rows : FIR<float | complex_t>, src/dsp/filter.h:51-74, batched -------- */
/* qdsp_hip_fir_cf32 / _f32 over nchan channel-major rows in one launch; kind 0 = float rows, 1 = complex_t rows; strides in
 * samples; real taps, one tap count per handle (1 <= ntaps <= 4096), every channel with its own tap values and its own history
 * (the last ntaps - 1 inputs of the row, 0 after create / reset), all on the device:
 *     y[c][i] = sum_k taps[c][k] x[c][i - (ntaps - 1) + k]
 * Every output component is the FP32 chain acc = fmaf(taps[c][k], x, acc) for k = 0 .. ntaps - 1 from +0.0f (row_fir_kernel): its
 * bits depend on the row's taps and the ntaps samples under them alone -- not on the call cuts, the row's place in the batch,
 * strides, alignment or the entry point -- and are those of qdsp_hip_fir_cf32 / _f32 in QDSP_HIP_FIR_DIRECT mode.  No zero taps
 * are padded in: a NaN at sample p reaches outputs p .. p + ntaps - 1 of its row and nothing else.
 * create loads the same taps into every channel.  set_taps: chan -1 = every channel, and ntaps may change, the history kept
 * and resized as qdsp_hip_fir_cf32_set_taps does (the newest samples preserved); chan >= 0 = that channel, ntaps must equal the
 * current count (else QDSP_HIP_EINVAL).  get_history / set_history: the ntaps - 1 samples of one channel, oldest first.
 * set_taps / get_history / set_history / reset synchronise the device and act from the next call.
 * process_batch_dev: asynchronous; device pointers aligned to the sample (4 / 8 bytes); 16-byte aligned output rows take the vector
 * stores.  d_in == d_out or spans that overlap are QDSP_HIP_EINVAL (a tile reads its neighbours' inputs).  count == 0 launches
 * nothing and keeps the history.  process_dev: the rows back to back.  process / process_ex (nchan 1): as for every
 * *_process_ex, `count` <= max_block where a side is on the host (else QDSP_HIP_ESIZE).
 * tile: the outputs per workgroup of row_fir_kernel; tap_group: the taps per unrolled group of its tap loop (what a test needs to
 * place its sizes around the kernel's boundaries). */
int qdsp_hip_rowfir_create(void** h, int device, int kind, int nchan, const float* taps, int ntaps, int max_block);
int qdsp_hip_rowfir_set_taps(void* h, int chan, const float* taps, int ntaps);
int qdsp_hip_rowfir_ntaps(void* h);
int qdsp_hip_rowfir_get_history(void* h, int chan, float* hist);
int qdsp_hip_rowfir_set_history(void* h, int chan, const float* hist);
int qdsp_hip_rowfir_process(void* h, const float* in, int count, float* out);
int qdsp_hip_rowfir_process_ex(void* h, const void* in, int in_link, int count, void* out, int out_link);
int qdsp_hip_rowfir_process_dev(void* h, const void* d_in, int64_t count, void* d_out, void* hip_stream);
int qdsp_hip_rowfir_process_batch_dev(void* h, const void* d_in, int64_t count, int64_t in_stride, void* d_out, int64_t out_stride,
                                      void* hip_stream);
int qdsp_hip_rowfir_reset(void* h);
void qdsp_hip_rowfir_destroy(void* h);
int qdsp_hip_rowfir_tile(void);
int qdsp_hip_rowfir_tap_group(void);

/* ---- DelayImag : src/dsp/processing.h:300-344 ------------------------------------------------ */
/* The one-sample Q delay of offset PSK over nchan complex_t rows: out[i] = {in[i].re, in[i - 1].im}, in[-1].im = the row's carried
 * lastIm (0 after create / reset; get_state / set_state, chan -1 = every channel).  Bit copies only (delay_imag_kernel): NaN
 * payloads and signed zeros pass unchanged.  Pointers 8-byte aligned; d_in == d_out or overlapping spans are QDSP_HIP_EINVAL (the
 * reference's loop may run in place; here a lane reads its neighbour's sample); count == 0 keeps the state.  Entry points as
 * for qdsp_hip_rowfir_*. */
int qdsp_hip_delay_imag_create(void** h, int device, int nchan, int max_block);
int qdsp_hip_delay_imag_get_state(void* h, int chan, float* last_im);
int qdsp_hip_delay_imag_set_state(void* h, int chan, float last_im);
int qdsp_hip_delay_imag_process(void* h, const float* in_iq, int count, float* out_iq);
int qdsp_hip_delay_imag_process_ex(void* h, const void* in, int in_link, int count, void* out, int out_link);
int qdsp_hip_delay_imag_process_dev(void* h, const void* d_in, int64_t count, void* d_out, void* hip_stream);
int qdsp_hip_delay_imag_process_batch_dev(void* h, const void* d_in, int64_t count, int64_t in_stride, void* d_out,
                                          int64_t out_stride, void* hip_stream);
int qdsp_hip_delay_imag_reset(void* h);
void qdsp_hip_delay_imag_destroy(void* h);

/* ---- PSKDemod<ORDER, OFFSET> and MSKDemod : src/dsp/demodulator.h:499-682 -------------------- */
/* A whole demodulator chain over nchan complex_t rows in one call, every intermediate on the device.  A chain handle owns one
 * handle of each stage and runs their *_process_batch_dev on the call's stream, one after the other:
 *   PSK (order 2 / 4 / 8, offset 0 / 1):  qdsp_hip_cagc (set point 1.0f, max gain 65535, agc_rate: PSKDemod::init) ->
 *        qdsp_hip_rowfir kind 1 (rrc_taps, the same for every channel until set) -> qdsp_hip_costas of that order, in place ->
 *        qdsp_hip_delay_imag (offset chains only) -> qdsp_hip_mmcr kind 1.  Symbols: complex_t.
 *   MSK:  qdsp_hip_demod QDSP_HIP_DEMOD_FM (sample_rate, deviation) -> qdsp_hip_mmcr kind 0.  Symbols: float.
 * so the symbols, counts and state are, bit for bit, those of the separate handles called in that order.  The parameters are
 * each stage's own and are checked by it (create returns the stage's error and leaves nothing allocated).
 * stage(which, &s): the BORROWED handle of a stage -- QDSP_HIP_PSK_AGC / _RRC / _COSTAS / _DELAY / _CLOCK, QDSP_HIP_MSK_FM / _CLOCK;
 * _DELAY on a chain without offset is QDSP_HIP_EINVAL.  Every per-channel setter and getter goes through it (qdsp_hip_cagc_set,
 * qdsp_hip_rowfir_set_taps, qdsp_hip_costas_set_bandwidth, qdsp_hip_mmcr_set_omega, ... and each stage's state).  A borrowed handle
 * is never processed on and never destroyed: it belongs to the chain and dies with it.
 * tap_dev(which, &rows, &stride): the device rows stage `which` wrote in the last call, `*stride` samples apart, 16-byte aligned,
 * valid until the next call on this handle; read them on that call's stream.  The intermediates share two scratch row sets, so
 * only rows that no later stage has overwritten are there: _COSTAS, _DELAY, _AGC of a chain without offset, and _FM; *rows is NULL
 * for _RRC (the Costas loop runs in place over them), for _AGC of an offset chain (the delay stage reuses them) and before the
 * first call; _CLOCK (its rows are the caller's) and _DELAY without offset are QDSP_HIP_EINVAL.
 * out_size(count) = the clock stage's qdsp_hip_mmcr_out_size, asked at call time.  process_batch_dev: asynchronous; d_in rows
 * 8-byte aligned, in_stride >= count; d_out, out_stride and d_counts as for qdsp_hip_mmcr_process_batch_dev.  count == 0 moves no
 * stage's state and clears the counts.  process_dev: the rows back to back (strides count and out_size(count)).  process /
 * process_ex (nchan 1) return the symbol count; the output link is QDSP_HIP_LINK_HOST or _DEVICE only, as for qdsp_hip_mmcr.
 * The scratch rows grow to the largest call seen (a call larger than max_block and every call before it synchronises the device
 * once).  reset resets every stage.  get_counts synchronises the device.  qdsp_hip_last_kernel reports the clock stage's launch. */
#define QDSP_HIP_PSK_AGC 0
#define QDSP_HIP_PSK_RRC 1
#define QDSP_HIP_PSK_COSTAS 2
#define QDSP_HIP_PSK_DELAY 3
#define QDSP_HIP_PSK_CLOCK 4
#define QDSP_HIP_MSK_FM 0
#define QDSP_HIP_MSK_CLOCK 1
int qdsp_hip_psk_create(void** h, int device, int order, int offset, int nchan, int max_block, const float* rrc_taps, int ntaps,
                        float agc_rate, float costas_bw, float omega, float gain_omega, float mu_gain, float rel_limit);
int qdsp_hip_psk_stage(void* h, int which, void** stage);
int qdsp_hip_psk_tap_dev(void* h, int which, void** d_rows, int64_t* stride);
int64_t qdsp_hip_psk_out_size(void* h, int64_t count);
int qdsp_hip_psk_process(void* h, const float* in_iq, int count, float* out_iq);
int qdsp_hip_psk_process_ex(void* h, const void* in, int in_link, int count, void* out, int out_link);
int qdsp_hip_psk_process_dev(void* h, const void* d_in, int64_t count, void* d_out, void* hip_stream);
int qdsp_hip_psk_process_batch_dev(void* h, const void* d_in, int64_t count, int64_t in_stride, void* d_out, int64_t out_stride,
                                   int* d_counts, void* hip_stream);
int qdsp_hip_psk_get_counts(void* h, int* counts);
int qdsp_hip_psk_reset(void* h);
void qdsp_hip_psk_destroy(void* h);
int qdsp_hip_msk_create(void** h, int device, int nchan, int max_block, float sample_rate, float deviation, float omega,
                        float gain_omega, float mu_gain, float rel_limit);
int qdsp_hip_msk_stage(void* h, int which, void** stage);
int qdsp_hip_msk_tap_dev(void* h, int which, void** d_rows, int64_t* stride);
int64_t qdsp_hip_msk_out_size(void* h, int64_t count);
int qdsp_hip_msk_process(void* h, const float* in_iq, int count, float* out);
int qdsp_hip_msk_process_ex(void* h, const void* in, int in_link, int count, void* out, int out_link);
int qdsp_hip_msk_process_dev(void* h, const void* d_in, int64_t count, void* d_out, void* hip_stream);
int qdsp_hip_msk_process_batch_dev(void* h, const void* d_in, int64_t count, int64_t in_stride, void* d_out, int64_t out_stride,
                                   int* d_counts, void* hip_stream);
int qdsp_hip_msk_get_counts(void* h, int* counts);
int qdsp_hip_msk_reset(void* h);
void qdsp_hip_msk_destroy(void* h);

/* ---- Threshold : src/dsp/processing.h:554-610 ------------------------------------------------ */
/* out[i] = (in[i] > 0.0f) ? 1 : 0 -- float rows in, uint8_t rows out, one byte per float, the same count; nchan channel-major rows
 * per call, in_stride in floats, out_stride in bytes (threshold_kernel).  NaN, -0.0f, +0.0f and negative denormals give 0; positive
 * denormals and +Inf give 1 (the compare is made on the bit pattern, whatever the denormal mode).  No state.  The reference's
 * setLevel / getLevel store a value its run() never reads: they exist in the C++ mirror only, with the same (non-)effect.
 * process_batch_dev: asynchronous; d_in 4-byte aligned, d_out any address (a lane's 16 outputs go out as one 16-byte store behind
 * the row's first 16-byte boundary, the bytes in front of it and the last partial group one by one); in_stride, out_stride >= count;
 * d_in_counts: int32[nchan] on the device or NULL (every row has `count`): row r converts min(max(d_in_counts[r], 0), count) floats
 * and leaves the rest of its output row untouched.  Spans of input and output that overlap are QDSP_HIP_EINVAL.  count == 0 launches
 * nothing.  process_dev: the rows back to back.  process / process_ex (nchan 1): link codes as for every *_process_ex, `count` <=
 * max_block where a side is on the host (else QDSP_HIP_ESIZE).  span: the outputs per workgroup of threshold_kernel. */
int qdsp_hip_threshold_create(void** h, int device, int nchan, int max_block);
int qdsp_hip_threshold_process(void* h, const float* in, int count, uint8_t* out);
int qdsp_hip_threshold_process_ex(void* h, const void* in, int in_link, int count, void* out, int out_link);
int qdsp_hip_threshold_process_dev(void* h, const void* d_in, int64_t count, void* d_out, void* hip_stream);
int qdsp_hip_threshold_process_batch_dev(void* h, const void* d_in, int64_t count, int64_t in_stride, const int* d_in_counts, void* d_out,
                                         int64_t out_stride, void* hip_stream);
void qdsp_hip_threshold_destroy(void* h);
int qdsp_hip_threshold_span(void);

/* ---- Deframer : src/dsp/deframing.h ------------------------------------------------------------ */
/* Sync-word framing over nchan channel-major rows of one bit per byte: search for the sync word, cut frames of frame_len bits and
 * pack them eight bits to a byte, MSB first.  kind 0 = uint8_t rows, kind 1 = float rows thresholded on load (x > 0 as for
 * qdsp_hip_threshold, so a demodulator's soft symbols need no byte row in between).  Per handle: frame_len in bits (1 .. 2^20) and
 * a sync word of sync_len bytes (1 .. 256), one bit per byte, compared as whole bytes like the reference's memcmp and shared by
 * the rows of the handle.  Per row, with x[p] the row's input bytes numbered from the last reset:
 *   d[q] = x[q - sync_len], d[q] = 0 for q < sync_len (the reference's zeroed work-buffer prefix);
 *   match(q) = (d[q .. q + sync_len) == sync word): it reads only inputs already received when position q is reached.
 * State per row: bits_read (-1 = searching), bad = 5, after = 0 after create / reset.  A call of n bytes advances q over n positions:
 *   reading (bits_read >= 0): frame bit k = bits_read is d[q]; it contributes (uint8_t)(d[q] << (7 - k % 8)), OR-ed into frame byte
 *     k / 8, every byte starting from 0 (input bytes other than 0 / 1 follow this formula); then q++, bits_read++; at bits_read ==
 *     frame_len the frame is emitted as frame_bytes = ceil(frame_len / 8) bytes, bits_read = -1, after = 1.
 *   after a frame (after): after = 0; if match(q), a frame starts at q with bad = 0; else if bad < 5, bad++ and a frame starts at q
 *     anyway (the reference's "try to save"); else search from q.
 *   searching: go to the smallest q' >= q with match(q'), bad = 0, a frame starts at q' (it includes the sync word); if there is no
 *     such q' among the positions received, remain searching.
 * This event form gives the frames of the reference's per-bit loop.  Departures from the reference: any count >= 0 is served (the
 * reference reads out of range below sync_len and copies count - 1 bytes, which is harmless there); the result is a function of
 * the concatenated row, whatever the call cuts; the sync word is shared by the rows of a handle; `after` reads back 0 while a frame
 * is being read (the reference leaves its flag set after a match, without effect).
 * A frame that spans calls is emitted by the call in which its last bit arrives; its earlier part is kept on the device.  A call
 * of `count` bytes emits at most out_size(count) = ceil(count / frame_len) frames per row.
 * set_sync: the same length only (else QDSP_HIP_EINVAL).  get_state / set_state: bits_read (-1 .. frame_len - 1), bad (0 .. 5),
 * after (0 / 1, and 0 while bits_read >= 0); chan -1 = every channel; the bytes of a frame in progress and the last sync_len
 * inputs are kept.  set_sync / get_state / set_state / reset / get_counts synchronise the device and act from the next call.
 * process_batch_dev: asynchronous; d_in_counts as for qdsp_hip_threshold (this is what lets the deframer follow qdsp_hip_mmcr_* and
 * qdsp_hip_{psk,msk}_process_batch_dev on the same stream with no host synchronisation); in_stride >= count, in input elements;
 * the frames of a row go back to back into its first slots, out_stride_bytes >= out_size(count) * frame_bytes, the bytes behind a
 * row's last frame are not touched; the per-row frame counts go to d_counts (int32[nchan], may be NULL) and to the handle
 * (get_counts).  kind 1: d_in 4-byte aligned.  Overlapping or equal d_in / d_out, a short stride and count > 2^30 are
 * QDSP_HIP_EINVAL.  count == 0 moves nothing, keeps the state and clears the counts.  Match words and frame starts live in
 * library-owned scratch sized for max_block at create (a larger device call grows it and synchronises the device once).
 * process_dev: the rows back to back (strides count and out_size(count) * frame_bytes).  process / process_ex (nchan 1) return the
 * frame count; `out` holds out_size(count) * frame_bytes bytes; the output link is QDSP_HIP_LINK_HOST or _DEVICE only, as for
 * qdsp_hip_mmcr; `count` <= max_block where a side is on the host (else QDSP_HIP_ESIZE).  tile / pack_span: the positions per
 * workgroup of deframe_match_kernel and of deframe_pack_kernel (at a frame_len that is a multiple of 8).  qdsp_hip_last_kernel
 * reports the match launch. */
int qdsp_hip_deframer_create(void** h, int device, int kind, int nchan, int max_block, int frame_len, const uint8_t* sync, int sync_len);
int qdsp_hip_deframer_set_sync(void* h, const uint8_t* sync, int sync_len);
int qdsp_hip_deframer_get_state(void* h, int chan, int* bits_read, int* bad, int* after);
int qdsp_hip_deframer_set_state(void* h, int chan, int bits_read, int bad, int after);
int64_t qdsp_hip_deframer_out_size(void* h, int64_t count);
int qdsp_hip_deframer_frame_bytes(void* h);
int qdsp_hip_deframer_process(void* h, const void* in, int count, uint8_t* out);
int qdsp_hip_deframer_process_ex(void* h, const void* in, int in_link, int count, void* out, int out_link);
int qdsp_hip_deframer_process_dev(void* h, const void* d_in, int64_t count, void* d_out, void* hip_stream);
int qdsp_hip_deframer_process_batch_dev(void* h, const void* d_in, int64_t count, int64_t in_stride, const int* d_in_counts, void* d_out,
                                        int64_t out_stride_bytes, int* d_counts, void* hip_stream);
int qdsp_hip_deframer_get_counts(void* h, int* counts);
int qdsp_hip_deframer_reset(void* h);
void qdsp_hip_deframer_destroy(void* h);
int qdsp_hip_deframer_tile(void);
int qdsp_hip_deframer_pack_span(void);

/* ---- Reed-Solomon decoder and FalconRS : src/dsp/falcon_fec.h, src/libcorrect/reed-solomon ------ */
/* Reed-Solomon decoding over GF(2^8) of interleaved frames, nchan channel-major rows of frames per call; every count of this
 * section is in FRAMES.  Stateless per frame.  Per handle: the primitive polynomial (9 bits, degree 8; one that is not primitive
 * is QDSP_HIP_EINVAL), first_root (0 .. 255), root_gap (gcd(root_gap, 255) = 1), num_roots (2 .. 32), the interleave depth I
 * (1 .. 8), skip (0 .. 64: bytes in front of the interleaved block, a sync word say), full_out (0 / 1) and optionally a 256-byte
 * input map, a 256-byte output map (NULL: the identity) and an XOR sequence of xor_len bytes, 1 .. 255 I (NULL: none).  Only
 * full-length codewords of 255 bytes.  A frame is frame_in_bytes = skip + 255 I bytes; with k = 255 - num_roots and d = in + skip:
 *   cw[c][p] = in_map[d[p I + c]], c < I, p < 255
 *   msg[c][0 .. k) = libcorrect's correct_reed_solomon_decode(cw[c], 255); the frame is good only if all I codewords decode
 *   out[i] = out_map[p < k ? msg[i % I][p] : 0] ^ xor[i % xor_len], p = i / I, for i < frame_out_bytes = (full_out ? 255 : k) I
 *   (full_out 1 is the reference block's: its output buffers keep their zeros behind byte k).
 * The decode is libcorrect's, bit for bit, also where it is not the textbook's.  With exp[i] = alpha^i, log[alpha^i] = i for
 * i = 1 .. 255 (so log 1 = 255) and coeff[i] = cw[254 - i]:
 *   S[i] = coeff(alpha^(root_gap (first_root + i))), i < num_roots; all zero: msg = cw[0 .. k), 0 symbols corrected.
 *   Locator: its Berlekamp-Massey loop (reed-solomon/decode.c:32-118), with its two coefficient arrays, its delay and the ORDER
 *     it tracks -- last order + delay where the register grows, the maximum of that and the order before where it does not; it is
 *     not the degree -- kept exactly; the discrepancy at step i runs over coefficients 1 .. numerrors.
 *   Roots: the x among all 256 elements with sum_{j <= order} Lambda[j] x^j = 0.  The codeword fails exactly when their number
 *     differs from the order.
 *   Per root x: the coefficient index is ((255 - log x) root_gap^-1) mod 255 (so 1 / x = 1 gives coefficient 0) and the value
 *     x^(first_root - 1) Omega(x) / Lambda'(x), Omega = S Lambda mod x^num_roots, Lambda' the formal derivative of the truncated
 *     locator, x / 0 = 0; the value is XOR-ed into the coefficient.  msg[i] = coeff[254 - i], i < k.
 *   A word with more than num_roots / 2 errors that this procedure takes to another codeword comes out as that codeword.
 *   One departure: an order equal to num_roots makes libcorrect read one byte past its table of powers; here the power is computed.
 * Good frames of a row go back to back into the row's first output slots, in input order; dropped frames leave no gap; the bytes
 * behind the last good frame are not touched.
 * process_batch_dev: asynchronous, three launches on hip_stream.  in_stride_bytes >= nframes * frame_in_bytes, out_stride_bytes >=
 * nframes * frame_out_bytes, any byte alignment of rows; d_in_counts: int32[nchan] on the device or NULL, row r has
 * min(max(d_in_counts[r], 0), nframes) frames (qdsp_hip_deframer's d_counts fits, so the two run on one stream with no host
 * synchronisation); d_counts: good frames per row, int32[nchan], may be NULL, also kept in the handle (get_counts); d_errs:
 * int32[nchan][nframes * I], may be NULL: per codeword -1 if it failed, else the symbols libcorrect corrected (the order its
 * locator search returned; 0 when the syndromes are zero); for a row shorter than nframes the entries behind its count are not
 * touched.  nframes == 0 moves nothing and clears the counts.  Overlapping d_in / d_out, a short stride and nframes > 2^22 are
 * QDSP_HIP_EINVAL.  Decoded frames pass through library-owned scratch sized for max_block frames at create (a larger device call
 * grows it and synchronises the device once).
 * process_dev: the rows back to back.  process / process_ex (nchan 1): `nframes` whole frames at `in`, `out` holds nframes *
 * frame_out_bytes; they return the good-frame count; the output link is QDSP_HIP_LINK_HOST or _DEVICE only; nframes <= max_block
 * where a side is on the host (else QDSP_HIP_ESIZE).  out_size(nframes) = nframes.  set_maps replaces the two maps and the XOR
 * sequence (NULL as at create), synchronises the device and acts from the next call; get_counts synchronises.
 * qdsp_hip_last_kernel reports the decode launch.
 * falcon_rs_create: the preset of dsp::FalconRS -- (0x187, 120, 11, 16), I = 5, skip = 4, full_out = 1, the CCSDS dual-basis maps
 * (in: from the dual basis, out: to it) and the CCSDS randomiser as the XOR sequence, all three computed from their closed forms. */
int qdsp_hip_rs_create(void** h, int device, int nchan, int max_block, int prim_poly, int first_root, int root_gap, int num_roots, int depth,
                       int skip, int full_out, const uint8_t* in_map, const uint8_t* out_map, const uint8_t* xor_seq, int xor_len);
int qdsp_hip_falcon_rs_create(void** h, int device, int nchan, int max_block);
int qdsp_hip_rs_set_maps(void* h, const uint8_t* in_map, const uint8_t* out_map, const uint8_t* xor_seq, int xor_len);
int64_t qdsp_hip_rs_out_size(void* h, int64_t nframes);
int qdsp_hip_rs_frame_in_bytes(void* h);
int qdsp_hip_rs_frame_out_bytes(void* h);
int qdsp_hip_rs_process(void* h, const uint8_t* in, int nframes, uint8_t* out);
int qdsp_hip_rs_process_ex(void* h, const void* in, int in_link, int nframes, void* out, int out_link);
int qdsp_hip_rs_process_dev(void* h, const void* d_in, int64_t nframes, void* d_out, void* hip_stream);
int qdsp_hip_rs_process_batch_dev(void* h, const void* d_in, int64_t nframes, int64_t in_stride_bytes, const int* d_in_counts, void* d_out,
                                  int64_t out_stride_bytes, int* d_counts, int* d_errs, void* hip_stream);
int qdsp_hip_rs_get_counts(void* h, int* counts);
void qdsp_hip_rs_destroy(void* h);

/* ---- FalconPacketSync : src/dsp/falcon_packet.h --------------------------------------------------- */
/* The last block of the Falcon 9 chain, behind FalconRS: nchan channel-major rows of frames per call, every result bit-exact.
 * An item is a frame; frames are frame_stride bytes apart (1195 .. 4096, a create parameter: with 1275 it reads the FalconRS
 * output in place); every count on the input side is in FRAMES.  Of a frame only bytes 0 .. 1194 are read: b0 .. b3, then
 * data[0 .. 1191).
 *   pkt = b3 | (b2 & 7) << 8 (11 bits), ctr = (b2 >> 3) | b1 << 5 | (b0 & 0x3f) << 13 (19 bits).
 * Per row the state is lastCounter (uint32, 0 after create / reset), packetRead (-1 after create / reset, otherwise 1 .. 16392)
 * and the packetRead pending bytes.  Per frame, in order:
 *   1. if uint32(lastCounter + 1) != ctr the pending packet is dropped (packetRead = -1); then lastCounter = ctr.  (The counter
 *      has 19 bits and the comparison 32: the wrap from 2^19 - 1 to 0 counts as a missed frame, as in the reference.)
 *   2. pkt == 2047, a continuation frame: if a packet is pending all 1191 data bytes are appended; nothing is emitted.
 *   3. otherwise, if a packet is pending, data[0 .. pkt) is appended and the pending packet is emitted with packetRead + pkt bytes
 *      (its own length field is not consulted); packetRead = -1.
 *   4. then (in every frame that is no continuation frame) the walk from i = pkt while i < 1191: if 1191 - i < 4 the bytes
 *      [i, 1191) become the pending packet and the walk ends; len = ((data[i] & 15) << 8 | data[i + 1]) + 2; len <= 2 ends the
 *      walk with nothing pending; if 1191 - i < len, [i, 1191) becomes the pending packet and the walk ends; otherwise
 *      data[i .. i + len) is emitted and i += len.
 *   Two departures, both where the reference reads or writes past a buffer.  Overflow: a pending packet never passes the
 *   reference's 0x4008 = 16392 bytes; an append that would pass it, in step 2 or 3, drops the pending packet instead (the
 *   reference writes past packet[]).  Bad pointer: a pkt of 1192 .. 2046 lies outside the data area; the pending packet is
 *   dropped, nothing is emitted and nothing becomes pending (the reference copies pkt bytes from a 1191-byte area).
 *   The reference's printf and its unused pktId read are not reproduced.
 * Output: the emitted packets of a row go back to back into the row's output bytes, in emission order; d_offs[row * offs_stride +
 * k] (int32) is the byte at which packet k begins and entry [count] the row's byte count, so a length is a difference;
 * d_counts[row] is the packet count.  Bytes and table entries behind those are not touched.  A call of n frames emits at most
 * out_packets(n) = 398 n packets per row (one pending packet and 1191 / 3 walked ones per frame; a header needs four bytes left,
 * so 396 walked ones are the most a frame reaches) and at most out_size(n) =
 * 16392 + 1191 n bytes (every emitted byte is a distinct data byte of the call or a carried one); n <= 2^20 per call, so offsets
 * fit int32.
 * The loop runs in its closed form.  The walk of step 4 starts with nothing pending whatever came before, so a frame f that is no
 * continuation frame determines by itself ctr_f, pkt_f, its walked packets data[pkt_f .. e_f) and its tail T_f: -1, or the residue
 * length 1191 - e_f.  With cont_f = (ctr_(f-1) + 1 == ctr_f) and g the nearest frame before f that is no continuation frame (or
 * the carried state), the incoming packetRead of f is in_f = T_g + 1191 (f - 1 - g) if T_g >= 0, cont holds for g + 1 .. f and the
 * sum does not pass 16392 (at most 13 continuation frames fit), else -1; f emits a pending packet exactly when in_f >= 0 and
 * in_f + pkt_f <= 16392, made of g's residue, the data areas of g + 1 .. f - 1 and data_f[0 .. pkt_f).  Two exclusive prefix sums
 * over the row, of packets and of bytes, place every frame's output.
 * process_batch_dev: asynchronous, three launches on hip_stream (fpkt_walk_kernel, fpkt_scan_kernel, fpkt_pack_kernel;
 * qdsp_hip_last_kernel reports the last).  in_stride_bytes >= (nframes - 1) * frame_stride + 1195, out_stride_bytes >=
 * out_size(nframes), offs_stride (in int32 entries) >= out_packets(nframes) + 1; rows may begin at any byte, d_offs is 4-byte
 * aligned; d_in_counts: int32[nchan] on the device or NULL, row r has min(max(d_in_counts[r], 0), nframes) frames (qdsp_hip_rs's
 * d_counts fits, so the two run on one stream with no host synchronisation); d_offs may be NULL and the offsets then go to a
 * table the library owns (offs_dev: its pointer, its row stride in entries and the device counts, valid until a call with more
 * frames than any before grows it; get_offsets copies up to cap + 1 entries of row `chan`, synchronises and returns the row's
 * packet count); d_counts may be NULL, the counts are also kept in the handle (get_counts: int32[2][nchan], packets and bytes).
 * d_out overlapping d_in, a short stride and nframes > 2^20 are QDSP_HIP_EINVAL.  nframes == 0 launches nothing, clears the
 * counts and leaves the state alone; a row with a count of 0 keeps its state and its pending packet.  State and pending bytes are
 * double-buffered.  Scratch is sized for max_block frames at create (a larger device call grows it and synchronises once).
 * process_dev: the rows back to back, in_stride_bytes = nframes * frame_stride, out_stride_bytes = out_size(nframes), the
 * library's offset table.  process / process_ex (nchan 1): `nframes` frames at `in`, `out` holds out_size(nframes) bytes; they
 * return the packet count, the offsets are the library's table's; the output link is QDSP_HIP_LINK_HOST or _DEVICE only;
 * nframes <= max_block where a side is on the host (else QDSP_HIP_ESIZE).
 * get_state (pending: QDSP_HIP_FPKT_MAX_PACKET bytes, may be NULL), set_state (chan -1: all rows; packet_read -1, or 1 .. 16392
 * with that many bytes at `pending`) and get_counts synchronise; reset restores the state after create.
 * A packet-sync handle given to a qdsp_hip_rs_* entry point, or a decoder's to one of these, is QDSP_HIP_EINVAL. */
#define QDSP_HIP_FPKT_FRAME_BYTES 1195
#define QDSP_HIP_FPKT_MAX_PACKET 16392
int qdsp_hip_fpkt_create(void** h, int device, int nchan, int max_block, int frame_stride);
int64_t qdsp_hip_fpkt_out_size(void* h, int64_t nframes);
int64_t qdsp_hip_fpkt_out_packets(void* h, int64_t nframes);
int qdsp_hip_fpkt_frame_stride(void* h);
int qdsp_hip_fpkt_process(void* h, const uint8_t* in, int nframes, uint8_t* out);
int qdsp_hip_fpkt_process_ex(void* h, const void* in, int in_link, int nframes, void* out, int out_link);
int qdsp_hip_fpkt_process_dev(void* h, const void* d_in, int64_t nframes, void* d_out, void* hip_stream);
int qdsp_hip_fpkt_process_batch_dev(void* h, const void* d_in, int64_t nframes, int64_t in_stride_bytes, const int* d_in_counts, void* d_out,
                                    int64_t out_stride_bytes, int* d_offs, int64_t offs_stride, int* d_counts, void* hip_stream);
int qdsp_hip_fpkt_offs_dev(void* h, int** d_offs, int64_t* stride, int** d_counts);
int qdsp_hip_fpkt_get_offsets(void* h, int chan, int* offs, int cap);
int qdsp_hip_fpkt_get_counts(void* h, int* counts);
int qdsp_hip_fpkt_get_state(void* h, int chan, uint32_t* last_counter, int* packet_read, uint8_t* pending);
int qdsp_hip_fpkt_set_state(void* h, int chan, uint32_t last_counter, int packet_read, const uint8_t* pending);
int qdsp_hip_fpkt_reset(void* h);
void qdsp_hip_fpkt_destroy(void* h);

/* ---- NOAA HRPT, TIP and HIRS demultiplexers : src/dsp/noaa/hrpt.h, src/dsp/noaa/tip.h ------------ */
/* The three blocks behind a Deframer(110900): nchan channel-major rows per call, every result bit-exact.  Bits are numbered MSB
 * first from the start of an item, as readBits does (src/dsp/utils/bitstream.h); bits(o, l) is the l-bit field at bit o.  In all
 * three, d_in_counts is int32[nchan] on the device or NULL: row r has min(max(d_in_counts[r], 0), count) items, so a Deframer's,
 * an HrptDemux's or a TipDemux's device counts feed the next stage on one stream with no host synchronisation.  Rows may begin at
 * any byte; uint16 outputs are 2-byte aligned; an output that overlaps the input, a short stride and a count above the stated
 * maximum are QDSP_HIP_EINVAL; count == 0 launches nothing and clears the counts.  Slots behind a row's count are not touched.
 * process / process_ex serve nchan 1 and count <= max_block where a side is on the host (else QDSP_HIP_ESIZE).
 *
 * HrptDemux (hrpt.h:36-78).  An item is a frame of 13863 bytes = 110900 bits = 11090 words of 10 bits, word(w) = bits(10 w, 10);
 * counts are in frames, at most 2^20 per row and call.  Stateless.
 *   AVHRR: d_avhrr[row * row_stride + c * plane_stride + frame * 2048 + p] = word(750 + 5 p + c), c < 5, p < 2048, strides in
 *     uint16 elements, plane_stride >= nframes * 2048: each (row, channel) is an image with one line per frame.  A line whose
 *     address is 16-byte aligned is written with 16-byte stores, any other with 2-byte stores.
 *   minor = bits(61, 2).  minor == 1: five TIP minor frames of 104 bytes, byte j of minor frame i = (word(103 + 104 i + j) >> 2)
 *     & 0xFF; minor == 3: the same bytes as five AIP minor frames; otherwise neither.  d_tip / d_aip: rows of minor frames back to
 *     back, compacted in frame order, strides in bytes >= nframes * 520; d_tip_counts / d_aip_counts: int32[nchan] on the device,
 *     in minor frames (what qdsp_hip_tip_process_batch_dev takes as d_in_counts); each of the five may be NULL and is skipped.
 *   process_batch_dev: asynchronous; hrpt_avhrr_kernel (one workgroup per frame), hrpt_scan_kernel and hrpt_gather_kernel on
 *     hip_stream.  process, process_ex, process_dev and qdsp_hip_time_process_dev are the single-output forms: rows of frames back
 *     to back in, the AVHRR planes out with plane_stride = nframes * 2048 and row_stride = 5 * nframes * 2048 (`avhrr` holds
 *     nframes * 10240 uint16); TIP and AIP go to device rows the library owns: tip_dev / aip_dev give the pointer, the row stride
 *     in bytes and the device counts (valid until a call with more frames than any before, which grows them), get_tip / get_aip
 *     copy up to `cap` minor frames of row `chan` to the host, synchronise and return the row's count.  get_frame_slots copies,
 *     for up to `cap` frames of row `chan` of the last call, where each frame's five minor frames went: -1 nowhere, s >= 0 with
 *     bit 30 clear: group s of the TIP row, bit 30 set: group s & 0x3fffffff of the AIP row (a group is 520 bytes); it
 *     synchronises and returns the row's frame count.  out_size(n) = n.
 *     get_counts: int32[3][nchan]: lines, TIP minor frames, AIP minor frames of the last call; synchronises.
 *     qdsp_hip_last_kernel reports the AVHRR launch.
 *
 * TipDemux (tip.h:31-124).  An item is a minor frame of 104 bytes; the output is one record of QDSP_HIP_TIP_RECORD_BYTES per
 * minor frame, HIRS[36] | SEM[2] | DCS[32] | SBUV[4] at the offsets below, each section the reference's byte list in its order.
 * Stateless; counts in minor frames, at most 2^24; strides in bytes; d_counts (may be NULL) receives the rows' counts.  One
 * launch, tip_kernel.  out_size(n) = n.
 *
 * HirsDemux (tip.h:136-238).  An item is a packet of 36 bytes; packets are packet_stride bytes apart (36 .. 4096, a create
 * parameter: with QDSP_HIP_TIP_RECORD_BYTES it reads TipDemux's records in place); counts in packets, at most 2^22.
 *   e = bits(19, 6).  Per row the state is lastElement (0 after create / reset), newImageData (0) and the line in progress, 20
 *   channels of 56 values (0xFFF).  Per packet, in order: if (e < lastElement || e > 55) && newImageData: the line is emitted and
 *   cleared, newImageData = 0; lastElement = e; if e <= 55: newImageData = 1 and value[ch][e] = u(bits(o[ch], 13)) with
 *   u(n) = n & 0x1000 ? 0x1000 + (n & 0xFFF) : 0xFFF - (n & 0xFFF) and o[] = 26 52 65 91 221 208 143 156 273 182 119 247 78 195 234
 *   260 39 104 130 169; if e == 55: the line is emitted and cleared, newImageData = 0.
 *   d_out[row * row_stride + ch * plane_stride + line * 56 + slot], strides in uint16 elements, plane_stride >= out_size(count)
 *   * 56; only emitted lines are written, d_counts (may be NULL) receives the rows' line counts; the line in progress stays in
 *   the handle.  out_size(n) = n + 1: both emissions can fall on the first packet after a set_state that no stream produces.
 *   The loop runs in its closed form: with e[-1] the carried lastElement, nid[0] the carried newImageData and nid[i] = e[i - 1]
 *   < 55, fb[i] = (e[i] < e[i - 1] || e[i] > 55) && nid[i], fa[i] = e[i] == 55, packet i writes line sum_{j < i} (fb[j] + fa[j])
 *   + fb[i], and of two packets in a row with one element in one line the later one counts.  Two launches, hirs_scan_kernel and
 *   hirs_pack_kernel; qdsp_hip_last_kernel reports the second.  State and the line in progress are double-buffered.
 *   process / process_ex / process_dev: plane_stride = (count + 1) * 56, row_stride = 20 * plane_stride; process and process_ex
 *   return the line count; the output link is QDSP_HIP_LINK_HOST or _DEVICE only.  get_state / set_state (chan -1: all rows;
 *   last_element 0 .. 63, new_image_data 0 / 1) and get_counts synchronise; reset restores the state after create. */
#define QDSP_HIP_TIP_RECORD_BYTES 74
#define QDSP_HIP_TIP_HIRS_OFFSET 0
#define QDSP_HIP_TIP_SEM_OFFSET 36
#define QDSP_HIP_TIP_DCS_OFFSET 38
#define QDSP_HIP_TIP_SBUV_OFFSET 70
int qdsp_hip_hrpt_create(void** h, int device, int nchan, int max_block);
int64_t qdsp_hip_hrpt_out_size(void* h, int64_t nframes);
int qdsp_hip_hrpt_process(void* h, const uint8_t* in, int nframes, uint16_t* avhrr);
int qdsp_hip_hrpt_process_ex(void* h, const void* in, int in_link, int nframes, void* avhrr, int out_link);
int qdsp_hip_hrpt_process_dev(void* h, const void* d_in, int64_t nframes, void* d_avhrr, void* hip_stream);
int qdsp_hip_hrpt_process_batch_dev(void* h, const void* d_in, int64_t nframes, int64_t in_stride_bytes, const int* d_in_counts, uint16_t* d_avhrr,
                                    int64_t row_stride, int64_t plane_stride, uint8_t* d_tip, int64_t tip_stride_bytes, int* d_tip_counts,
                                    uint8_t* d_aip, int64_t aip_stride_bytes, int* d_aip_counts, void* hip_stream);
int qdsp_hip_hrpt_get_counts(void* h, int* counts);
int qdsp_hip_hrpt_tip_dev(void* h, void** d_tip, int64_t* stride_bytes, int** d_counts);
int qdsp_hip_hrpt_aip_dev(void* h, void** d_aip, int64_t* stride_bytes, int** d_counts);
int qdsp_hip_hrpt_get_tip(void* h, int chan, uint8_t* out, int cap);
int qdsp_hip_hrpt_get_aip(void* h, int chan, uint8_t* out, int cap);
int qdsp_hip_hrpt_get_frame_slots(void* h, int chan, int* slots, int cap);
void qdsp_hip_hrpt_destroy(void* h);
int qdsp_hip_tip_create(void** h, int device, int nchan, int max_block);
int64_t qdsp_hip_tip_out_size(void* h, int64_t count);
int qdsp_hip_tip_process(void* h, const uint8_t* in, int count, uint8_t* out);
int qdsp_hip_tip_process_ex(void* h, const void* in, int in_link, int count, void* out, int out_link);
int qdsp_hip_tip_process_dev(void* h, const void* d_in, int64_t count, void* d_out, void* hip_stream);
int qdsp_hip_tip_process_batch_dev(void* h, const void* d_in, int64_t count, int64_t in_stride_bytes, const int* d_in_counts, void* d_out,
                                   int64_t out_stride_bytes, int* d_counts, void* hip_stream);
int qdsp_hip_tip_get_counts(void* h, int* counts);
void qdsp_hip_tip_destroy(void* h);
int qdsp_hip_hirs_create(void** h, int device, int nchan, int max_block, int packet_stride);
int64_t qdsp_hip_hirs_out_size(void* h, int64_t count);
int qdsp_hip_hirs_packet_stride(void* h);
int qdsp_hip_hirs_process(void* h, const uint8_t* in, int count, uint16_t* out);
int qdsp_hip_hirs_process_ex(void* h, const void* in, int in_link, int count, void* out, int out_link);
int qdsp_hip_hirs_process_dev(void* h, const void* d_in, int64_t count, void* d_out, void* hip_stream);
int qdsp_hip_hirs_process_batch_dev(void* h, const void* d_in, int64_t count, int64_t in_stride_bytes, const int* d_in_counts, uint16_t* d_out,
                                    int64_t row_stride, int64_t plane_stride, int* d_counts, void* hip_stream);
int qdsp_hip_hirs_get_counts(void* h, int* counts);
int qdsp_hip_hirs_get_state(void* h, int chan, int* last_element, int* new_image_data);
int qdsp_hip_hirs_set_state(void* h, int chan, int last_element, int new_image_data);
int qdsp_hip_hirs_reset(void* h);
void qdsp_hip_hirs_destroy(void* h);

/* ---- stereo FM : StereoFMDemod, src/dsp/demodulator.h:189-330 ------------------------------ */
/* Complex rows in, stereo_t {l, r} rows out; nchan channel-major rows per call, strides in samples, each channel with its own
 * phasorSpeed, carried phase, pilot-filter history and AGC level, all kept on the device.  One call is one run() of the
 * reference (which has no PLL and no loop over samples but the FM phase), as three launches on one stream:
 *   m = FloatFMDemod(in), bit-identical to QDSP_HIP_DEMOD_FM with the same phase (fm_demod_kernel).
 *   f[i] = sum_k pilot_taps[k] m[i - (ntaps - 1) + k]: FIR<float>, the tap convention and the (ntaps - 1)-sample history of
 *        qdsp_hip_fir_f32, the history 0 after create / reset (pilot_fir_kernel).  Each output is the FP32 chain
 *        acc = fmaf(taps[k], m[..], acc) for k = 0 .. ntaps - 1 from +0.0f: its bits depend on the taps and the ntaps samples under
 *        them alone, not on where the stream is cut into calls, on the channel index or count, or on the alignment of the rows.
 *        The reference's taps are BlackmanBandpassWindow(1000, 1000, 19000, sampleRate); ntaps <= 4096, shared by all channels.
 *   level: AGC's update exactly as stated for qdsp_hip_agc_* above, on f, with cfr = 20.0f / sample_rate (demodulator.h:219):
 *        the decay in dB by cfr * count, then the maximum of the call's f under `x > level`.  0 after create / reset.
 *   p = f * (1.0f / level);  d = p * p;  s = m * d;  out = {m + s, m - s}, every operation rounded to float (stereo_mix_kernel).
 *        Bit-identical to the reference's VOLK lines given m, f and the level; AGC's corner cases are kept (a level of 0 with no
 *        positive f gives p = f * inf; an Inf pins the level; a NaN never raises it).  As in the reference, the filter's delay is
 *        not compensated: m is not delayed against p.
 * A NaN input sample at i makes m[i] and m[i + 1] NaN, hence the outputs i .. i + ntaps of that channel and no others.
 * set_fm(chan, sample_rate, deviation): phasorSpeed as qdsp_hip_demod_set_fm, and cfr; default sample_rate = deviation = 1; a
 * sample_rate that is not finite and positive is QDSP_HIP_EINVAL.  `chan` -1 = every channel (set_fm, set_phase, set_level).
 * set_pilot_taps replaces the taps of all channels and zeroes the history -- a departure: FIR<float>::updateWindow keeps the
 * old samples -- and leaves phase and level alone.  pilot_dev: the device rows of f of the last call, `*stride` floats apart,
 * 16-byte aligned, valid until the next call on this handle (NULL before the first); read them on the stream of that call.
 * process / process_ex (nchan 1): host pointers / link codes as for every *_process_ex, `count` <= max_block where a side is on
 * the host (else QDSP_HIP_ESIZE).  process_dev: the nchan rows back to back (strides = count).  Device pointers 8-byte aligned;
 * 16-byte aligned rows with even strides take the vector loads and stores.  count == 0 is a no-op.  QDSP_HIP_EINVAL: ntaps < 1
 * or > 4096, nchan > 65535, spans of input and output that overlap.  m and f live in library-owned rows that grow to the largest
 * call seen (a call larger than max_block and every call before it synchronises the device once).  get_* synchronise the device. */
int qdsp_hip_stereo_fm_create(void** h, int device, int nchan, const float* pilot_taps, int ntaps, int max_block);
int qdsp_hip_stereo_fm_set_fm(void* h, int chan, float sample_rate, float deviation);
int qdsp_hip_stereo_fm_set_pilot_taps(void* h, const float* pilot_taps, int ntaps);
int qdsp_hip_stereo_fm_process(void* h, const float* in_iq, int count, float* out_lr);
int qdsp_hip_stereo_fm_process_ex(void* h, const void* in, int in_link, int count, void* out, int out_link);
int qdsp_hip_stereo_fm_process_dev(void* h, const void* d_in, int64_t count, void* d_out, void* hip_stream);
int qdsp_hip_stereo_fm_process_batch_dev(void* h, const void* d_in, int64_t count, int64_t in_stride, void* d_out,
                                         int64_t out_stride, void* hip_stream);
int qdsp_hip_stereo_fm_get_phase(void* h, int chan, float* phase);
int qdsp_hip_stereo_fm_set_phase(void* h, int chan, float phase);
int qdsp_hip_stereo_fm_get_level(void* h, int chan, float* level);
int qdsp_hip_stereo_fm_set_level(void* h, int chan, float level);
int qdsp_hip_stereo_fm_pilot_dev(void* h, void** d_pilot, int64_t* stride);
int qdsp_hip_stereo_fm_reset(void* h);
void qdsp_hip_stereo_fm_destroy(void* h);

/* ---- synthetic IQ source (measurement harness) ------------------------------ */
/* Counter-based uniform [-1,1) per float component, generated on device so benchmarks are
 * HBM->HBM.  Bit-identical to oracle_synth_iq() for the same (first_sample, seed). */
int qdsp_hip_synth_iq_dev(int device, void* d_out_iq, int64_t first_sample, int64_t count,
                          uint32_t seed, void* hip_stream);

/* ---- introspection for the measurement harness ----------------------------------------- */
/* ---- Viterbi decoder : src/libcorrect/convolutional (correct_convolutional_decode / _decode_soft) ---- */
/* The decoder of libcorrect's convolutional codes over nchan channel-major rows of terminated frames; every count of this section
 * is in FRAMES, every result bit-exact.  Stateless: nothing is carried from frame to frame or call to call, and there are no
 * setters.  Per handle: rate (2 or 3), order (6 .. 9), `rate` polynomials below 2^order, sets (order + 7 .. 65536: the groups of
 * `rate` symbols of a frame) and soft (0 / 1); anything else is QDSP_HIP_EINVAL.  A frame is frame_in_bytes = sets * rate soft
 * bytes (0 a strong zero, 255 a strong one), or ceil(sets * rate / 8) bytes of hard bits, MSB first; it comes out as
 * frame_out_bytes = (sets - order + 1) / 8 bytes, MSB first.  Each frame is decoded exactly as a FRESHLY CREATED
 * correct_convolutional decodes it (correct_convolutional_decode_soft(conv, in, sets * rate, out) / _decode: a reused object carries
 * its renormalisation counter from call to call; here the counter is 0 at every frame start):
 *   table[r] = sum_i parity(r & poly[i]) << i over the `order`-bit register r; 2^(order-1) states; state j has predecessors
 *   j >> 1 (low, label table[j]) and (j >> 1) | 2^(order-2) (high, label table[j | 2^(order-1)]).
 *   Branch metric of label x: soft sum_i |y[i] - (x >> i & 1 ? 255 : 0)| (CORRECT_SOFT_LINEAR); hard popcount(x ^ g), bit i of g
 *   the i-th bit of the group.  Path metrics are uint16_t and wrap: each sum is cut to 16 bits before it is compared.
 *   Sets 1 .. order - 2 (warm-up): metric[j] = branch(table[j]) + metric[j >> 1] from zeros; no decision is recorded.  Set 0 is
 *   read and counts for nothing: error_buffer_swap takes its read side before it moves its index, so the first swap after a reset
 *   changes nothing and what set 0 wrote is overwritten by set 1.
 *   Then sets - order + 1 processed steps.  Inner steps take the low predecessor when low <= high.  The last order - 1 steps (the
 *   tail) take it only when low < high, and the k-th of them (k = 1 ..) considers only states that are multiples of skip = 2^k.
 *   After processed step n: if n is a multiple of floor(65535 / (255 rate)) (128 / 85), the best state -- least metric among
 *   every skip-th (1 outside the tail), the lowest index at the minimum -- is searched and its metric subtracted from all; if the
 *   history holds 20 order steps (n = 20 order + 15 order m), a traceback from the best state (the same search, after the
 *   subtraction) walks 5 order steps back and emits the 15 order decisions before them.  After the last step a traceback from
 *   state 0 emits every decision still held.  Decision bits are written MSB first; the trailing partial byte is not stored.
 *   (Where every searched metric is 65535 the C code reads an uninitialised index; here the lowest searched state is taken.)
 * process_batch_dev: asynchronous, one launch (viterbi_decode_kernel, one wave per frame) on hip_stream.  in_stride_bytes >=
 * nframes * frame_in_bytes, out_stride_bytes >= nframes * frame_out_bytes, rows and frames at any byte alignment; d_in_counts:
 * int32[nchan] on the device or NULL, row r has min(max(d_in_counts[r], 0), nframes) frames (qdsp_hip_deframer's d_counts fits:
 * the two run on one stream with no host synchronisation); the output of frames behind a row's count is not touched.
 * nframes == 0 moves nothing.  Overlapping d_in / d_out, a short stride and nframes > 2^22 are QDSP_HIP_EINVAL.
 * process_dev: the rows back to back.  process / process_ex (nchan 1): `nframes` whole frames at `in`; link codes as for the
 * Reed-Solomon decoder; nframes <= max_block where a side is on the host (else QDSP_HIP_ESIZE); they return 0.
 * The handle is known by its address, in a set of its own: every entry point refuses a handle of any other kind, a destroyed
 * decoder, a second destroy and foreign memory, without reading the pointer.  qdsp_hip_last_kernel reports the launch. */
int qdsp_hip_viterbi_create(void** h, int device, int nchan, int max_block, int rate, int order, const uint16_t* poly, int sets, int soft);
int qdsp_hip_viterbi_frame_in_bytes(void* h);
int qdsp_hip_viterbi_frame_out_bytes(void* h);
int qdsp_hip_viterbi_process(void* h, const uint8_t* in, int nframes, uint8_t* out);
int qdsp_hip_viterbi_process_ex(void* h, const void* in, int in_link, int nframes, void* out, int out_link);
int qdsp_hip_viterbi_process_dev(void* h, const void* d_in, int64_t nframes, void* d_out, void* hip_stream);
int qdsp_hip_viterbi_process_batch_dev(void* h, const void* d_in, int64_t nframes, int64_t in_stride_bytes, const int* d_in_counts, void* d_out,
                                       int64_t out_stride_bytes, void* hip_stream);
void qdsp_hip_viterbi_destroy(void* h);

/* Name of the kernel the last process* call of this handle launched, and its launch
 * geometry; used by bench.py to pick the right row out of a rocprofv3 kernel trace. */
int qdsp_hip_last_kernel(void* h, char* name, int name_len, int* grid, int* block, int* lds_bytes);
/* Time `iters` back-to-back process_dev launches of this handle on `hip_stream` with HIP
 * events recorded on that same stream; returns mean milliseconds per launch in *ms.
 * State advances as for `iters` ordinary calls. */
int qdsp_hip_time_process_dev(void* h, const void* d_in, int64_t count, void* d_out,
                              void* hip_stream, int iters, float* ms);

/* ---- ring: the halo exchange of the time-sharded path over RCCL / xGMI ----------------------------------
 * The reference has no multi-device path (one thread per block: src/dsp/block.h:83-85).  A long stream is cut into time chunks over
 * the GPUs of a node, one process per GPU; a chunk's filter needs the last H INPUT samples of the chunk before it in the stream --
 * the samples src/dsp/filter.h:71 / src/dsp/resampling.h:129 carry from one run() to the next.  Every step each rank posts
 *     ncclGroupStart(); ncclSend(my tail -> rank + 1); ncclRecv(rank - 1's tail); ncclGroupEnd();
 * on the ring's own HIP stream and installs what arrives with <op>_set_history_dev.  A C++ graph (qdsp_amd/host/examples/
 * graph_check.cpp `shard`) and qdsp_amd/sharding.py RingStream call the same five entry points.
 *   available  1 when RCCL could be bound in this process (dlopen of librccl.so.1), else 0: lets every rank vote BEFORE the
 *              collective create (a ring with one end missing would hang; qdsp_amd/sharding.py takes that vote)
 *   unique_id  one rank (rank 0) obtains the 128-byte id; the caller carries it to every rank (file, socket, MPI, a torch store)
 *   create     collective: every rank of the ring calls it with the same id; world 1 = the rank is its own neighbour
 *   post       my tail (halo_bytes at d_tail, as of what `producer_stream` has queued so far) -> rank + 1, and rank - 1's tail ->
 *              the next of four receive buffers; returns at once.  At most two posts may be outstanding.
 *   complete   `consumer_stream` waits for the oldest outstanding post; *d_halo = what arrived with it, *d_prev_halo = what
 *              arrived with the post before it (zeros before the first): in a block-cyclic cut rank 0's predecessor is the LAST
 *              rank of the step before.  Either pointer may be NULL.
 *   drain      host-side wait for everything posted (end of stream: every rank has one exchange in flight that no step reads;
 *              also: call it before a collective of ANOTHER communicator of the same process, e.g. a torch.distributed barrier)
 *   info       what the communicator itself reports: ncclCommCount / ncclCommUserRank / ncclCommCuDevice and the RCCL version
 *              code (-1 where the bound RCCL lacks the query) -- evidence for a scaling run, not needed by the data path
 *   set_timing / exchange_us   optional: HIP timing events around each send/recv group on the ring stream; mean / max duration
 *              in microseconds of the exchanges finished so far (includes waiting for the neighbour to post its end)
 * Lifetimes (one consumer stream per ring):
 *   d_tail        must stay unmodified until the matching complete(): work queued on consumer_stream AFTER that complete may
 *                 overwrite it (the send is ordered before the event complete waits for).
 *   *d_halo       valid for work queued on consumer_stream between this complete() and the next but one complete();
 *   *d_prev_halo  ... between this complete() and the next one.  The ring waits for that work (an event recorded on
 *                 consumer_stream by each complete) before a later post receives into the same buffer.  Work on another
 *                 stream must be ordered behind consumer_stream by the caller.
 * Errors: QDSP_HIP_ERCCL when librccl.so.1 cannot be loaded or an RCCL call fails (its message goes to stderr). */
#define QDSP_HIP_RING_ID_BYTES 128
int qdsp_hip_ring_available(void);
int qdsp_hip_ring_unique_id(void* id);
int qdsp_hip_ring_create(void** ring, int device, int rank, int world, const void* id, int halo_bytes);
int qdsp_hip_ring_post(void* ring, const void* d_tail, void* producer_stream);
int qdsp_hip_ring_complete(void* ring, void* consumer_stream, const void** d_halo, const void** d_prev_halo);
int qdsp_hip_ring_drain(void* ring);
int qdsp_hip_ring_info(void* ring, int* comm_ranks, int* comm_rank, int* comm_device, int* rccl_version);
int qdsp_hip_ring_set_timing(void* ring, int on);
int qdsp_hip_ring_exchange_us(void* ring, double* mean_us, double* max_us, long long* exchanges);
void qdsp_hip_ring_destroy(void* ring);

#ifdef __cplusplus
}
#endif
#endif /* QDSP_HIP_H */
