/*
 * nsh_hip.h -- C-ABI of libnsh_hip.so, the MI355X (gfx950) kernel shim behind the
 * newsched block-execution path.
 *
 * Plain C, POD arguments only (device pointers as void* or float*, sizes as size_t/int64_t,
 * streams and events as opaque void*). No C++ or torch types cross this boundary, so the
 * newsched C++17 host (meson or otherwise) links it directly, and Python reaches it with
 * ctypes.
 *
 * Every entry point returns 0 on success or a nonzero hipError_t-style code; it never
 * throws. The text of the last failure on the calling thread is in nsh_last_error().
 * The C++ wrappers (gr::hip_buffer, gr::hip::* blocks) turn nonzero codes into
 * std::runtime_error, because WORK_ERROR would spin forever in the reference executor
 * (schedulers/mt/lib/graph_executor.cpp:102-131).
 *
 * Reference interfaces each group replaces (paths relative to the reference tree):
 *   streams/events     cudaStreamCreate per buffer/block (runtime/lib/cudabuffer.cu:37,
 *                      blocklib/cuda/lib/copy.cpp:33) and cudaStreamSynchronize per work()
 *                      (copy.cpp:58, cudabuffer.cu:175) -> one stream per GPU partition,
 *                      event-ordered edges, no host syncs in steady state.
 *   ring memory        cuda_buffer's 2x cudaMalloc + mirror copies (cudabuffer.cu:27-35,
 *                      :116-176) -> one HIP-VMM allocation mapped twice back to back.
 *   nsh_memcpy_async   cuda_buffer::post_write H2D/D2H copies (cudabuffer.cu:129-157) and
 *                      copy_items (cudabuffer.cu:179-183, a host memcpy on device memory).
 *   nsh_copy           apply_copy_kernel (blocklib/cuda/lib/copy.cu:6-33), one launch per
 *                      1024-sample vector (copy.cpp:49-57) -> one launch per work().
 *   nsh_mul_const_*    multiply_const_kernel (blocklib/cuda/lib/multiply_const.cu:1-18, ff
 *                      only) and the CPU multiply_const<T>::work (blocklib/blocks/lib/
 *                      multiply_const.cpp:17-46, VOLK 32fc_s32fc / 32f_s32f).
 *   nsh_add_cc, nsh_mul_cc, nsh_fir_*, nsh_fft1024_c2c, nsh_channelizer1024
 *                      no reference counterpart; GNU Radio semantics.
 */
#ifndef NSH_HIP_H
#define NSH_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define NSH_ABI_VERSION 1

/* ---- errors / device ---------------------------------------------------------- */
int nsh_abi_version(void);
const char* nsh_last_error(void);          /* thread-local; "" when no error */
int nsh_get_device_count(int* count);
int nsh_set_device(int dev);
int nsh_device_info(int dev, int* n_cu, int* clock_khz, size_t* hbm_bytes, char* arch, int arch_len);
int nsh_device_sync(void);
/* PCI bus id of `dev` ("dddd:bb:dd.f"): identifies a physical GPU across processes whose
 * device ordinals differ (per-rank HIP_VISIBLE_DEVICES makes every rank device 0). */
int nsh_device_pci_id(int dev, char* buf, int len);
/* *device = the GPU whose memory `ptr` points into (hipPointerGetAttributes, device memory
 * only: VMM rings and hipMalloc), else -1 (NULL, pinned or pageable host memory). The rccl
 * transport checks every buffer with it before handing it to librccl, so a wrong pointer is a
 * thrown error of the edge instead of a fault inside an RCCL kernel. */
int nsh_pointer_device(const void* ptr, int* device);

/* ---- streams and events (opaque hipStream_t / hipEvent_t) ---------------------- */
int nsh_stream_create(int dev, void** stream);
int nsh_stream_destroy(void* stream);
int nsh_stream_sync(void* stream);
/* 0: every operation on the stream has finished; 1: not yet; -1: error (hipStreamQuery, no wait). */
int nsh_stream_query(void* stream);
int nsh_event_create(void** event);
int nsh_event_destroy(void* event);
int nsh_event_record(void* event, void* stream);
int nsh_event_query(void* event);          /* 0 complete, 1 not ready, <0 error */
int nsh_event_sync(void* event);
int nsh_event_elapsed_ms(void* start, void* stop, float* ms);
int nsh_stream_wait_event(void* stream, void* event);
/* Times the NEXT kernel launched by this library on the calling thread (e.g. the FIR kernel of
 * the next nsh_fir_ccf / nsh_fir_cascade_ccf): the launch records start_event when the kernel
 * begins and stop_event when it ends, as part of its own dispatch (hipExtLaunchKernel), instead
 * of two event records around the call -- two fewer stream packets per timed launch. Events from
 * nsh_event_create. The setting is consumed by that one launch; (NULL, NULL) clears it. Replaces
 * the per-work() cudaEventRecord pairs a CUDA block would use for kernel timing (the reference
 * blocks do not time their kernels). */
int nsh_time_next_launch(void* start_event, void* stop_event);
/* (Every kernel entry point takes an armed pair with its launch and drops it, unrecorded, if it
 * returns without launching: the stream kernels, fft / channelizer, synth, FIR and cascade.)
 * Launches on the calling thread so far that recorded a pair set by nsh_time_next_launch (a pair
 * spanning several launches of one entry point counts each launch that records one of its two
 * events). A caller that armed a pair compares the count before and after the call it meant to
 * time: unchanged means no launch took the pair (the call launched nothing; the pair was dropped
 * unrecorded when the entry point returned). gr::schedulers::scheduler_hip's kernel timing. */
int nsh_timed_launches(uint64_t* count);
/* The shader clock while other work runs: one wave on `stream` (meant to be a second stream beside
 * the measured kernel's) reads the SQ cycle counter and the 100 MHz real-time counter, sleeps for
 * real_ticks (<= 2^32) ticks of the latter, reads both again and writes {cycles, ticks} to out_dev
 * (2 x uint64, device memory): MHz = 100 * cycles / ticks. The wave's end is bounded by the real-
 * time counter and by an iteration cap. A measurement helper (bench.py records the clock each
 * timed leg ran at); no reference counterpart. */
int nsh_clock_sample(void* out_dev, int64_t real_ticks, void* stream);

/* ---- memory ----------------------------------------------------------------------- */
enum nsh_copy_kind { NSH_H2D = 0, NSH_D2H = 1, NSH_D2D = 2, NSH_DEFAULT = 3 };
int nsh_malloc(int dev, size_t bytes, void** ptr);
int nsh_free(void* ptr);
int nsh_host_alloc(size_t bytes, void** ptr);       /* pinned, device-visible */
int nsh_host_free(void* ptr);
int nsh_memcpy_async(void* dst, const void* src, size_t bytes, int kind, void* stream);
int nsh_memset_async(void* ptr, int value, size_t bytes, void* stream);

/* Device ring for gr::hip_buffer: one physical allocation of *actual_bytes (>= min_bytes,
 * rounded to the VMM granularity) mapped twice back to back, so [base, base+2*actual)
 * aliases [base, base+actual) -- read_ptr()/write_ptr() spans are always contiguous and
 * no mirror copy is ever made. *double_mapped = 0 means VMM was unavailable and a plain
 * allocation was returned; the caller must then cap spans at the wrap point. */
int nsh_ring_alloc(int dev, size_t min_bytes, void** base, size_t* actual_bytes, int* double_mapped);
int nsh_ring_free(void* base);

/* Inter-process device memory: the "p2p" transport of gr::domain_adapter_remote (a flowgraph
 * edge between two processes whose rings are device memory). The receiving process exports a
 * nsh_malloc'd landing area (nsh_ipc_mem_export -> NSH_IPC_HANDLE_BYTES opaque bytes sent over
 * the edge's control socket); the sending process maps it on its own device
 * (nsh_ipc_mem_open) and writes it with a stream-ordered nsh_memcpy_async (same GPU: a local
 * D2D copy; different GPUs: a peer write over xGMI). Replaces the reference's direct
 * peer-buffer access between domains, which exists only inside one process
 * (runtime/include/gnuradio/domain_adapter_direct.hpp:156-172); the reference has no
 * cross-process edge. */
#define NSH_IPC_HANDLE_BYTES 64
int nsh_ipc_mem_export(void* dev_ptr, void* handle_out);
int nsh_ipc_mem_open(int dev, const void* handle, void** ptr);
int nsh_ipc_mem_close(void* ptr);

/* ---- stream kernels (n counts complex samples unless the name ends in _ff) --------- */
int nsh_copy(const void* in, void* out, size_t bytes, void* stream);
int nsh_mul_const_cc(const float* in, float* out, int64_t n, float k_re, float k_im, void* stream);
int nsh_mul_const_ff(const float* in, float* out, int64_t n, float k, void* stream);
/* m multiply_const_cc stages fused into one pass: k holds m (re,im) pairs, applied in
 * order with the same per-stage float rounding as m separate launches. */
int nsh_mul_const_chain_cc(const float* in, float* out, int64_t n, const float* k_host, int m, void* stream);
int nsh_add_cc(const float* a, const float* b, float* out, int64_t n, void* stream);
int nsh_mul_cc(const float* a, const float* b, float* out, int64_t n, void* stream);
/* multiply_const_vcc: items of vlen complex samples, y[i][j] = x[i][j] * k[j], k_dev a device
 * array of vlen (re,im) pairs (GNU Radio's vector-constant multiply; the reference has only the
 * scalar multiply_const<T> over n_items*vlen, blocklib/blocks/lib/multiply_const.cpp:33-46). */
int nsh_mul_const_vcc(const float* in, float* out, const float* k_dev, int vlen, int64_t nitems, void* stream);

/* Counter-based synthetic stream: x[i] = (u(2i), u(2i+1)),
 * u(j) = 24-bit uniform in [-1,1) from splitmix64(seed ^ j), j counted from first_index*2. */
int nsh_synth_cf32(float* out, int64_t n, uint64_t first_index, uint64_t seed, void* stream);

/* ---- FIR (fir_filter_ccf, optionally decimating) ----------------------------------
 * y[m] = sum_{k<ntaps} h[k] * x[m*decim - k], x complex fp32, h real fp32. The block keeps
 * its own (ntaps-1)-sample history because the reference block API has none
 * (runtime/include/gnuradio/sync_block.hpp:36-86). Per call:
 *   in       : n_out*decim input samples (device)
 *   hist_in  : ntaps-1 samples that precede in[0] (device; zeros at stream start; NULL = zeros,
 *              which saves the stream-start memset)
 *   hist_out : receives the ntaps-1 samples that precede the NEXT call's in[0]
 *              (must not alias hist_in -- ping-pong two buffers; NULL is an error, returned
 *              before any launch, except for NSH_FIR_PFFT plans, which then skip it)
 * NULL in / out or a NULL plan return an error before any launch.
 * algo: NSH_FIR_AUTO picks by measurement (MFMA for decim 1, 2, 4 with finite
 * taps, PFFT for decim 8 and 16, else DIRECT); NSH_FIR_DIRECT is the fp32 VALU direct form
 * (decim 1, 2, 4, 8); NSH_FIR_MFMA is the split-precision Toeplitz form on the matrix
 * cores: decim 1 on 32-sample blocks, ntaps <= 161, fp16x2 at a per-chunk power-of-two scale
 * with three products (k_fir_mfma12); decim 2 and 4 as the polyphase fp16x2 form
 * (k_fir_mfma13, the XCD-lockstep walk; NSH_DEC_WALK_MASK=0 selects k_fir_mfma11, the contiguous
 * walk). In both, a 2048-input chunk whose samples (with its halo) are finite but span
 * more than the split holds takes the exact-fp32 matrix tile of NSH_FIR_MFMA_F32 (fp32 products
 * and sums; the decimators filter it undecimated and keep every decim-th output), and one
 * holding inf/NaN the fp32 direct form (exact IEEE semantics) -- in a second kernel
 * the call enqueues right after the first on the same stream (k_fir_exact12 / k_fir_exact13 filter
 * the chunks k_fir_mfma12 / k_fir_mfma13 queued; they return at once when none were); k_fir_mfma11
 * filters such chunks inside its own launch. A plan may be used on several streams (each has its own queue of such chunks); its
 * first call on a stream, or a call with more chunks than any before on that stream, allocates
 * that queue (the latter after synchronizing the stream);
 * NSH_FIR_MFMA16 (3) and NSH_FIR_MFMA_BF16X3 (4) name bf16x3 kernels retired in round 4: plan
 * creation refuses them; NSH_FIR_MFMA_F32 is the exact-fp32 Toeplitz form on the fp32-input matrix instructions
 * (decim 1, ntaps <= 257, finite taps; no operand split: fp32 products and sums, chunks with
 * inf/NaN through the fp32 direct form in the same launch). NSH_FIR_PFFT (decim 8 and 16; AUTO
 * picks it there when ceil((ntaps-1)/decim) <= 256 and the taps are finite): the polyphase-FFT
 * overlap-save kernel of nsh_fir_cascade_ccf with one stage (k_fir_pfft2<16> / k_fir_pfft<8,1>; within fp32
 * transform rounding of the direct form, frame-relative, see nsh_fir_cascade_ccf below); decim 16
 * is only available as PFFT. */
enum nsh_fir_algo {
    NSH_FIR_AUTO = 0,
    NSH_FIR_DIRECT = 1,
    NSH_FIR_MFMA = 2,
    NSH_FIR_MFMA16 = 3,
    NSH_FIR_MFMA_BF16X3 = 4,
    NSH_FIR_MFMA_F32 = 5,
    NSH_FIR_PFFT = 6
};
int nsh_fir_plan_create(int dev, const float* taps_host, int ntaps, int decim, int algo, void** plan);
int nsh_fir_plan_destroy(void* plan);
int nsh_fir_plan_algo(void* plan);          /* the algorithm AUTO resolved to */
const char* nsh_fir_plan_kernel(void* plan); /* the kernel nsh_fir_ccf launches, e.g. "k_fir_mfma12<5>" */
int nsh_fir_ccf(void* plan, const float* in, const float* hist_in, float* hist_out,
                float* out, int64_t n_out, void* stream);

/* Decimating FIR chain in one pass (the fused form of nstages fir_filter_ccf(h_s, D_s) blocks in
 * a chain; BASELINE config C5 = 4 x fir_filter_ccf(firwin(127, 0.45), 2); replaces nstages
 * nsh_fir_ccf calls and the intermediate streams). The chain composes into one decimating filter
 *   y[m] = sum_n heq[n] x[m D - n],   D = prod D_s,   heq = h_1 * (h_2 up D_1) * (h_3 up D_1 D_2) ...
 * (composed in double at plan creation), computed by polyphase-FFT overlap-save
 * (k_fir_pfft2<16> / k_fir_pfft<8,1>; ceil((len(heq) - 1) / D) <= 256). Per call: in = n_out * D
 * samples; hist_in / hist_out = nsh_fir_cascade_hist_len(plan) = len(heq) - 1 input samples, as
 * for nsh_fir_ccf (NULL hist_in reads as zeros; hist_out may be NULL; no aliasing). A chain whose
 * stages all start from zero history is equivalent to this plan from a zero history.
 * Accuracy (not bit-identical to the staged chain): fp32 transform rounding, relative to each
 * 512-row frame's input level rather than to each output -- per output
 *   |y - y_chain| <= 1e-5 |y_chain| + 1e-6 max|x over the output's frame window| sum|heq|
 * (C5 on the synthetic stream: 2.2e-7 of max|y| against the oracle's double-accumulated chain;
 * north-star tolerance 1e-5). So quiet outputs that share a frame (8192 inputs at D = 16) with a
 * much louder burst are accurate to the burst's level, not their own
 * (tests/test_gpu_pfft.py::test_c5_mixed_amplitude_frame_relative_bound).
 * The frame window of output m of a call is inputs [D (f V - Q), D (f V - Q) + 512 D), f = m / V,
 * Q = ceil((len(heq) - 1) / D), V = 512 - Q (the call's history before input 0). The frame is scaled
 * by an exact power of two taken from that window (k_fir_pfft2<16>) or, in k_fir_pfft<P,1>, from
 * inputs [D (f - 1) V, D (f + 1) V), which add the V - Q rows before the window: a stretch there
 * more than about 2^100 louder than the whole window pushes the window into fp32's subnormals.
 * tests/test_gpu_pfft_taps.py holds every output to the bound above on full-size asymmetric taps,
 * impulses, scale exponents from -110 to 125 and inf/NaN frames at three and four frames per workgroup.
 * Frames holding inf/NaN are computed by the staged chain itself (fp32 direct form, stage by
 * stage over the frame's window): their NaN and inf outputs are the chain's exactly. That holds for
 * chains of 2 to 8 stages whose first two stage outputs over one window fit the kernel's image
 * buffers: n1 + n2 <= 571 D, n1 = ceil(512 D / D_1), n2 = ceil(n1 / D_2) -- every chain that starts
 * with a decimating stage, and e.g. (h, 1) -> (g, 16). Every other plan runs the fp32 direct form on
 * heq for such frames, which can give +-inf where the chain's inf - inf gives NaN: a one-stage plan
 * (heq is its taps), a chain of more than 8 stages, and a chain that does not fit, e.g.
 * (h, 1) -> (g, 2) -> (k, 8), or (h, 1) -> (g, 8) at D = 8
 * (tests/test_gpu_pfft_taps.py::test_nonfinite_plan_variants). */
int nsh_fir_cascade_plan_create(int dev, const float* const* taps_host, const int* ntaps, const int* decims,
                                int nstages, void** plan);
int nsh_fir_cascade_plan_destroy(void* plan);
int nsh_fir_cascade_decim(void* plan);         /* D = prod D_s */
int nsh_fir_cascade_hist_len(void* plan);      /* len(heq) - 1 */
const char* nsh_fir_cascade_kernel(void* plan); /* "k_fir_pfft2<16>" (D = 16; "k_fir_pfft<16,1>" with NSH_PFFT_FORM=1), "k_fir_pfft<8,1>" */
int nsh_fir_cascade_ccf(void* plan, const float* in, const float* hist_in, float* hist_out, float* out,
                        int64_t n_out, void* stream);

/* ---- rotator_cc and freq_xlating_fir_filter_ccf (no reference counterpart; GNU Radio semantics) ----
 * Phase: a frequency is a 64-bit fixed-point phase increment in turns per sample,
 *   inc = round(frac(t) * 2^64) mod 2^64   (exact from the double t; negative t wraps),
 * and the phase of absolute stream sample n is (n * inc) mod 2^64 turns in plain uint64 wrap-around
 * arithmetic: independent of how the stream is cut into calls and of the stream position.
 *   nsh_phase_inc      host only; refuses a non-finite frequency.
 *   nsh_rotate_cc      y[i] = x[i] * exp(+j 2 pi phase(first_index + i)); one launch (k_rotate) per
 *                      call whatever n and the 8-byte pointer alignment; in == out is allowed.
 *   nsh_fir_xlat_ccf   with inc = phase_inc(-freq_norm), freq_norm = center_freq / samp_rate:
 *                        y[m] = sum_{k<ntaps} h[k] * (x[m*decim - k] * exp(j 2 pi phase(first_index + m*decim - k)))
 *                      (= GNU Radio's freq_xlating_fir_filter_ccf: a signal at +center_freq lands at
 *                      DC), 1 <= decim <= 64, 1 <= ntaps <= 1024, one launch of the fused kernel
 *                      k_fir_xlat<R,S> (rotate at staging, fp32 direct form, decimate). History as
 *                      nsh_fir_ccf: hist_in = the ntaps-1 RAW (unrotated) samples before in[0], i.e.
 *                      stream samples first_index - (ntaps-1) + j mod 2^64 (NULL = zeros); hist_out
 *                      receives the last ntaps-1 raw samples bit-exactly and must not alias hist_in.
 *                      Non-finite samples propagate by plain IEEE arithmetic.
 * Argument errors (NULL pointers, ntaps or decim out of range, a non-finite frequency, aliased
 * history) are refused before any HIP call; n <= 0 / n_out <= 0 return 0 and launch nothing.
 * Measured (DESIGN.md section 4.3, 127 taps): the fused kernel is the faster form from decimation 8
 * upward; at decimation 1, 2 and 4 the staged nsh_rotate_cc -> nsh_fir_ccf(AUTO) is (the MFMA FIR). */
int nsh_phase_inc(double turns_per_sample, uint64_t* inc);
int nsh_rotate_cc(const float* in, float* out, int64_t n, uint64_t phase_inc, uint64_t first_index, void* stream);
int nsh_fir_xlat_plan_create(int dev, const float* taps_host, int ntaps, int decim, double freq_norm, void** plan);
int nsh_fir_xlat_plan_destroy(void* plan);
int nsh_fir_xlat_phase_inc(void* plan, uint64_t* inc);       /* = phase_inc(-freq_norm) */
int nsh_fir_xlat_tile(void* plan);                           /* outputs per workgroup of the chosen instantiation */
const char* nsh_fir_xlat_kernel(void* plan);                 /* e.g. "k_fir_xlat<4,2>" */
int nsh_fir_xlat_ccf(void* plan, const float* in, const float* hist_in, float* hist_out, float* out,
                     int64_t n_out, uint64_t first_index, void* stream);

/* ---- pfb_channelizer_ccf: critically sampled M-channel polyphase filterbank (GNU Radio semantics) ----
 * nchans = M channels (a power of two in [2, 64]), h = taps_host: the real fp32 prototype low-pass
 * with ntaps = L taps (1 <= L <= 1024, ceil(L / M) <= 32), x the complex fp32 input stream. Output
 * time step m, channel c (0 <= c < M):
 *   y[m][c] = sum_{k<L} h[k] * x[m*M - k] * exp(+j 2 pi c k / M)
 * Channel c is the band centred at +c/M cycles per sample, moved to DC, filtered by h and decimated
 * by M: channel 0 is DC, channels above M/2 are the negative frequencies (GNU Radio's channel
 * order). Column c equals nsh_fir_xlat_ccf with decim = M, freq_norm = c/M, first_index = 0 and the
 * same history. Computed in polyphase form, k = p + q*M:
 *   u_p[m]  = sum_q h[p + q*M] * x[(m-q)*M - p]           (M branch FIRs of ceil(L / M) taps)
 *   y[m][c] = sum_{p<M} u_p[m] * exp(+j 2 pi c p / M)     (unnormalised inverse DFT, radix 2)
 * Per call (one launch of k_pfb<M>): in = n_out*M samples; out = n_out items of M complex samples,
 * time-major and channel-minor (what a vlen-M port carries). History as nsh_fir_ccf: hist_in = the
 * L-1 raw samples before in[0] (NULL = zeros); hist_out receives the last L-1 raw samples
 * bit-exactly, must not alias hist_in and is required when L > 1. in, out and the histories need
 * only 8-byte alignment (out is stored 16 bytes wide when it is 16-byte aligned).
 * Accuracy: fp32 throughout, exact twiddle constants (computed in double on the host). The DFT mixes
 * the branches, so errors are relative to the largest channel of the data compared (a few 1e-7 of
 * it), not to each channel: a quiet channel beside a loud one is accurate to the loud one's level.
 * Non-finite samples propagate by IEEE arithmetic: a time step whose L-tap window holds a NaN is NaN
 * in all M channels; taps beyond L (the padding up to ceil(L / M) * M) are skipped, never multiplied,
 * so no other time step is.
 * Argument errors (NULL pointers, nchans not a power of two in [2, 64], ntaps outside [1, 1024], more
 * than 32 taps per branch, aliased history, a NULL plan, a missing hist_out) are refused before any
 * HIP call; n_out <= 0 returns 0 and launches nothing.
 * Measured (one MI355X, 2^26 inputs, kernel times): 56 to 74 % of 8 TB/s on
 * 16 B per input sample, 1.1 to 1.5 times nsh_copy's time over the same bytes, and 5.8 (M = 4) to 57
 * (M = 64) times faster than the M nsh_fir_xlat_ccf launches that produce the same channels. */
int nsh_pfb_plan_create(int dev, const float* taps_host, int ntaps, int nchans, void** plan);
int nsh_pfb_plan_destroy(void* plan);                 /* NULL: 0 */
int nsh_pfb_tile(void* plan);                         /* time steps per workgroup; 0 for NULL */
const char* nsh_pfb_kernel(void* plan);               /* e.g. "k_pfb<16>"; "" for NULL */
int nsh_pfb_channelizer_ccf(void* plan, const float* in, const float* hist_in, float* hist_out, float* out,
                            int64_t n_out, void* stream);

/* ---- pfb_synthesizer_ccf: critically sampled M-channel synthesis filterbank, the channelizer's counterpart ----
 * nchans = M channels (a power of two in [2, 64]), h = taps_host: the real fp32 prototype low-pass
 * with ntaps = L taps (1 <= L <= 1024, Q = ceil(L / M) <= 32), used as given: no gain of M (scale the
 * taps by M for unity gain, as with an interpolating FIR). The input is a stream of items of M complex
 * fp32 samples, time-major and channel-minor, X[m][c]: what nsh_pfb_channelizer_ccf emits and a vlen-M
 * port carries. The output is a complex stream at M times the item rate:
 *   y[n] = sum_{c<M} sum_{m'} X[m'][c] * h[n - m'*M] * exp(+j 2 pi c n / M)      (0 <= n - m'*M < L)
 * Every channel is zero-stuffed by M, filtered by h and moved to +c/M cycles per sample, and the M
 * results are summed; the channel order is the channelizer's (channel 0 is DC, channels above M/2 the
 * negative frequencies). This is not GNU Radio's block of the name (M separate streams, a 2x mode, a
 * channel map). Computed in polyphase form, n = m*M + r:
 *   v_r[m]     = sum_{c<M} X[m][c] * exp(+j 2 pi c r / M)    (unnormalised inverse DFT, radix 2)
 *   y[m*M + r] = sum_{q<Q, r+q*M<L} h[r + q*M] * v_r[m - q]  (M branch FIRs of at most Q taps)
 * Per call (one launch of k_pfb_synth<M>): in = n_in items (n_in*M samples); out = n_in*M samples.
 * History: hist_in = the Q-1 raw input items, (Q-1)*M samples, before in[0] (NULL = zeros); hist_out
 * receives the last Q-1 raw items bit-exactly, must not alias hist_in and is required when Q > 1; with
 * Q = 1 there is no history. in, out and the histories need only 8-byte alignment (out is stored 16
 * bytes wide when it is 16-byte aligned).
 * Accuracy: fp32 throughout, exact twiddle constants (computed in double on the host). The DFT mixes
 * the channels, so errors are relative to the loudest channel, not to each. Non-finite samples
 * propagate by IEEE arithmetic: taps at or past L (the padding up to Q*M) are skipped, never
 * multiplied, so a NaN in any channel of item m' makes exactly the L outputs [m'*M, m'*M + L - 1] NaN.
 * Argument errors (NULL pointers, nchans not a power of two in [2, 64], ntaps outside [1, 1024], more
 * than 32 taps per branch, aliased history, a NULL plan, a missing hist_out) are refused before any
 * HIP call; n_in <= 0 returns 0 and launches nothing.
 * Measured (one MI355X, 2^26 outputs, kernel times): 51 to 75 % of 8 TB/s on
 * 16 B per output sample, 1.07 to 1.59 times nsh_copy's time over the same bytes, 0.98 to 1.09 times
 * k_pfb<M> at the same filter, and 11 (M = 4) to 165 (M = 64) times faster than the M nsh_resamp_ccf,
 * M nsh_rotate_cc and M - 1 nsh_add_cc launches that produce the same stream. */
int nsh_pfb_synth_plan_create(int dev, const float* taps_host, int ntaps, int nchans, void** plan);
int nsh_pfb_synth_plan_destroy(void* plan);           /* NULL: 0 */
int nsh_pfb_synth_tile(void* plan);                   /* items per workgroup; 0 for NULL */
const char* nsh_pfb_synth_kernel(void* plan);         /* e.g. "k_pfb_synth<16>"; "" for NULL */
int nsh_pfb_synthesizer_ccf(void* plan, const float* in, const float* hist_in, float* hist_out, float* out,
                            int64_t n_in, void* stream);

/* ---- rational_resampler_ccf: resample by interp / decim (GNU Radio semantics) ----
 * interp = I, decim = D (1 <= I, D <= 64, used as given, not reduced by their gcd), h = taps_host: the
 * real fp32 low-pass with ntaps = L taps (1 <= L <= 1024), x the complex fp32 input stream. Zero-stuff
 * by I, filter, keep every D-th sample:
 *   y[n] = sum_{k<L} h[k] * u[n*D - k],   u[j*I] = x[j], u = 0 elsewhere
 *        = sum_{q<Q} h[phi + q*I] * x[j0 - q],   phi = (n*D) mod I, j0 = floor(n*D / I), Q = ceil(L / I)
 * (D = 1 is interp_fir_filter_ccf, I = 1 fir_filter_ccf with decimation D). Larger ratios such as
 * 160/147, and rates that are no ratio at all, are nsh_arb_resamp_ccf's (the next section).
 * Per call (one launch of k_resamp<R,P>): n_units units, each D inputs and I outputs: in = n_units*D
 * samples, out = n_units*I samples, so every call starts at phase 0 and the only state is the history.
 * History as nsh_fir_ccf, but Q-1 samples (nsh_resamp_history): hist_in = the Q-1 raw samples before
 * in[0] (NULL = zeros); hist_out receives the last Q-1 raw samples bit-exactly, must not alias hist_in
 * and is required when Q > 1. in, out and the histories need only 8-byte alignment (out is stored 16
 * bytes wide when it is 16-byte aligned).
 * Accuracy: fp32, q ascending, one FMA per component and tap: the order is fixed per output, so the
 * results are bit-identical however the stream is cut into calls. Taps at or beyond L (the padding up
 * to Q*I) are skipped, never multiplied: a non-finite sample reaches exactly the outputs whose L-tap
 * sum holds it.
 * Argument errors (NULL pointers, ntaps, interp or decim out of range, aliased history, a NULL plan, a
 * missing hist_out) are refused before any HIP call; n_units <= 0 returns 0 and launches nothing.
 * Measured (one MI355X, 2^27 samples in and out together, kernel times): 2.2 to
 * 2.8 times nsh_copy's time over the same 8 (n_in + n_out) bytes at (2, 1), (4, 1), (3, 2), (2, 3),
 * (4, 5) and (64, 1), 29 to 37 % of 8 TB/s; the pure decimators (1, 4, 127 taps) and (1, 64, 1024 taps)
 * take 0.97 and 2.0 times nsh_fir_xlat_ccf at frequency 0 on the same data. */
int nsh_resamp_plan_create(int dev, const float* taps_host, int ntaps, int interp, int decim, void** plan);
int nsh_resamp_plan_destroy(void* plan);              /* NULL: 0 */
int nsh_resamp_tile(void* plan);                      /* units per workgroup; 0 for NULL */
const char* nsh_resamp_kernel(void* plan);            /* e.g. "k_resamp<8,1>"; "" for NULL */
int nsh_resamp_history(void* plan);                   /* Q - 1; 0 for NULL */
int nsh_resamp_ccf(void* plan, const float* in, const float* hist_in, float* hist_out, float* out,
                   int64_t n_units, void* stream);

/* ---- pfb_arb_resampler_ccf: resample by an arbitrary rate (GNU Radio's pfb_arb_resampler) ----
 * nfilt = F filters (a power of two in [2, 64]; GNU Radio's default is 32), h = taps_host: the real
 * fp32 prototype with ntaps = L taps (1 <= L <= 2048; Q = ceil(L / F) taps per filter), rate = r output
 * samples per input sample, finite, 1/64 <= r <= 64; x the complex fp32 input stream. The plan computes
 * the derivative taps in fp32 on the host, d[k] = fl32(h[k+1] - h[k]) for k < L-1 and d[L-1] = 0 (GNU
 * Radio's create_diff_taps).
 * Phase: exact integer arithmetic in place of GNU Radio's float accumulator, so the output does not
 * depend on how the stream is cut into calls. step = round(F / r * 2^32) (nsh_arb_step; exact from the
 * double, ties to even) is a uint64 in Q32.32 counted in filter steps; a phase, in the same format, is
 * the position of a call's output 0 relative to in[0]. Output n of the call is at
 *   pos(n) = phase + n*step            (exact, unbounded)
 *   k(n) = pos(n) >> 32,  i(n) = k(n) div F,  j(n) = k(n) mod F,
 *   mu(n) = float((pos(n) & 0xffffffff) >> 8) * 2^-24     (24 bits: exactly representable)
 *   y[n] = sum_{q : j + q*F < L} (h[j + q*F] + mu * d[j + q*F]) * x[i(n) - q]
 * (filter j plus mu times derivative filter j). Taps at k >= L (the padding up to Q*F) are skipped,
 * never multiplied: a non-finite sample reaches exactly the outputs whose window holds it.
 * A call has n_in inputs and makes n_out outputs; it needs i(n_out - 1) <= n_in - 1. nsh_arb_span gives
 *   *n_out      = min(want_out, ceil((n_in*F*2^32 - phase) / step) when that is positive, else 0),
 *   *n_consumed = c = min(i(*n_out), n_in),     *phase_next = pos(*n_out) - c*F*2^32,
 * and the next call starts at in + c with phase_next and the history this call wrote. n_out = 0 with
 * n_in > 0 is a valid, advancing call: it consumes c inputs and hands the history on (a decimator
 * whose next output lies beyond the items it was given).
 * nsh_arb_step and nsh_arb_span are host only and make no HIP call. nsh_arb_span refuses a step that
 * is not that of a rate in [1/64, 64] for this nfilt and n_in or want_out outside [0, 2^31 - 1].
 * History as nsh_fir_ccf, but Q-1 samples (nsh_arb_history): hist_in = the Q-1 raw samples before in[0]
 * (NULL = zeros); hist_out receives the Q-1 raw samples before in[c] bit-exactly, must not alias
 * hist_in and is required when Q > 1. in, out and the histories need only 8-byte alignment (out is
 * stored 16 bytes wide when it is 16-byte aligned). One launch of k_arb<R,P> per call (none for an
 * advancing call with Q = 1).
 * Accuracy: fp32 throughout, in a fixed order per output: q ascending, w = fmaf(mu, d, h), then one
 * FMA per component, acc = fmaf(w, x, acc). The results are bit-identical however the stream is cut
 * into calls (with phase and history chained).
 * Argument errors (NULL pointers, nfilt not a power of two in [2, 64], ntaps outside [1, 2048], a rate
 * that is not finite or outside [1/64, 64], aliased history, a missing hist_out, a NULL plan, an n_out
 * larger than nsh_arb_span allows for (phase, n_in), n_in or n_out above 2^31 - 1) are refused before
 * any HIP call; n_in <= 0 returns 0 and launches nothing.
 * Measured: DESIGN.md section 4.6. */
int nsh_arb_step(double rate, int nfilt, uint64_t* step);
int nsh_arb_span(uint64_t step, int nfilt, uint64_t phase, int64_t n_in, int64_t want_out, int64_t* n_out,
                 int64_t* n_consumed, uint64_t* phase_next);
int nsh_arb_plan_create(int dev, const float* taps_host, int ntaps, int nfilt, double rate, void** plan);
int nsh_arb_plan_destroy(void* plan);                 /* NULL: 0 */
int nsh_arb_tile(void* plan);                         /* outputs per workgroup; 0 for NULL */
const char* nsh_arb_kernel(void* plan);               /* e.g. "k_arb<4,1>"; "" for NULL */
int nsh_arb_history(void* plan);                      /* Q - 1; 0 for NULL */
int nsh_arb_plan_step(void* plan, uint64_t* step);    /* = nsh_arb_step(rate, nfilt) */
int nsh_arb_resamp_ccf(void* plan, const float* in, int64_t n_in, const float* hist_in, float* hist_out, float* out,
                       int64_t n_out, uint64_t phase, void* stream);

/* ---- FFT(fft_vcc, 1024-point, unnormalised both ways) ------------------------------
 * frames of 1024 complex samples; inverse=1 computes sum_k X[k] e^{+2 pi i kn/1024}
 * (= 1024 * numpy.fft.ifft). nsh_channelizer1024 fuses fft -> multiply by w[1024]
 * (complex, device) -> ifft in one pass over HBM, bit-identical to nsh_fft1024_c2c ->
 * nsh_mul_const_vcc(vlen 1024) -> nsh_fft1024_c2c(inverse) (the scheduler's fusion relies on it).
 * in, out and w need only 8-byte alignment (one complex sample; results are bit-identical to the
 * 16-byte aligned call); in and out must not alias. Exactly nframes * 1024 samples are read and
 * written for any nframes >= 1.
 * Frames are independent: a frame's output depends on that frame's samples alone, bit for bit,
 * whatever the batch size and its place in it; a non-finite sample makes all 1024 outputs of its
 * own frame non-finite (NaN in both parts for a nan+nanj sample) and touches no other frame. Which
 * part turns NaN and which inf is not specified.
 * Scaling the input by a power of two scales the output by it exactly, as long as nothing
 * overflows or turns subnormal (the growth is at most 1024 sqrt(2) per transform).
 * Argument errors (NULL in / out / w, in == out) are refused before any HIP call; nframes <= 0
 * returns 0 and launches nothing, whatever the pointers. */
int nsh_fft1024_c2c(const float* in, float* out, int64_t nframes, int inverse, void* stream);
int nsh_channelizer1024(const float* in, float* out, const float* w, int64_t nframes, void* stream);

/* ---- FFT plan (fft_vcc of any power-of-two size 16..8192, windowed and shifted) --------
 * Frames of fft_size complex samples, forward or inverse, unnormalised both ways, with an optional
 * real window of fft_size floats (host; copied) on the input and an optional half-frame shift, in
 * one launch: every sample crosses HBM once each way. With w[n] = 1 when window_host is NULL:
 *   forward  X[k] = sum_n x[n] w[n] e^{-2 pi i kn/N};  shift: out[k] = X[(k + N/2) mod N]
 *   inverse  y[n] = x[n] w[n] (the window indexed by the input position as it arrives);
 *            shift: y'[n] = y[(n + N/2) mod N];  out[m] = sum_n y'[n] e^{+2 pi i mn/N}
 *            (= N * numpy.fft.ifft of y').
 * The window product is one fp32 multiply per component, the shift an index change on the store
 * (forward) or the load (inverse): the shifted output is bit-identical to the swapped halves of the
 * unshifted one, and an all-ones window to none. A plan of size 1024 without window and shift runs
 * the kernel of nsh_fft1024_c2c (same bits).
 * nsh_fft_c2c runs on the current device, which must be the plan's. in and out need only 8-byte
 * alignment (results are bit-identical to the 16-byte aligned call); they must not alias. Exactly
 * nframes * fft_size samples are read and written for any nframes >= 1.
 * Frames are independent: a frame's output depends on that frame's samples alone, bit for bit,
 * whatever the batch size, the frame's slot in its wave or workgroup (nsh_fft_tile frames share a
 * workgroup, up to 64 a wave) and the grid cap; a non-finite sample makes all fft_size outputs of
 * its own frame non-finite and touches no other frame.
 * Scaling the input (or the window) by a power of two scales the output by it exactly, as long as
 * nothing overflows or turns subnormal.
 * nsh_fft_plan_grid_cap bounds the workgroups of the grid-stride walk over the frames (0 restores
 * the default); the output does not depend on it.
 * Refused before any HIP call: an fft_size that is not a power of two in [16, 8192], a NULL plan
 * out-pointer, a non-finite window entry, a NULL plan / in / out at run time, in == out, a negative
 * cap. nframes <= 0 returns 0 and launches nothing, whatever the other arguments. An armed
 * nsh_time_next_launch pair is taken by the one launch (dropped when nothing is launched).
 * Measured: DESIGN.md section 4.7. */
int nsh_fft_plan_create(int dev, int fft_size, int inverse, const float* window_host /* NULL: none */, int shift,
                        void** plan);
int nsh_fft_plan_destroy(void* plan);                 /* NULL: 0 */
int nsh_fft_plan_size(void* plan);                    /* fft_size; 0 for NULL */
int nsh_fft_tile(void* plan);                         /* frames per workgroup; 0 for NULL */
const char* nsh_fft_kernel(void* plan);               /* e.g. "k_fft<4096, false, false>"; "" for NULL */
int nsh_fft_plan_grid_cap(void* plan, int max_workgroups);
int nsh_fft_c2c(void* plan, const float* in, float* out, int64_t nframes, void* stream);

/* ---- fft_filter_ccc: FIR filter with complex taps by overlap-save (GNU Radio's fft_filter_ccc) ----
 * h = taps_host: ntaps = L complex fp32 taps as (re, im) pairs, 1 <= L <= 4096; x the complex fp32
 * input stream; decimation 1:
 *   y[n] = sum_{k<L} h[k] * x[n-k]
 * History as nsh_fir_ccf: hist_in = the L-1 raw samples before in[0] (NULL = zeros); hist_out
 * receives the last L-1 raw samples of hist_in ++ in bit-exactly, must not alias hist_in and is
 * required when L > 1.
 * Frames: N = fft_size in {1024, 2048, 4096, 8192} with L <= N/2; 0 lets the plan choose: 1024 up
 * to 256 taps, 2048 up to 512, 4096 up to 2048, 8192 above (the smallest N >= 4 * pow2ceil(L) up to
 * 4096, the smallest N >= 2 * pow2ceil(L) beyond; pow2ceil: the next power of two at or above).
 * V = N - (L-1) valid outputs per frame: frame f of a call owns out[fV, (f+1)V) up to n and reads
 * the window of inputs [fV-(L-1), fV-(L-1)+N); window positions below 0 come from the history (or
 * are zeros), positions at or past n are zeros, nothing at or past out[n] is stored. One launch of
 * k_fft_xlat<N, 1, false> per call: window -> forward FFT -> times Hs -> inverse FFT -> store of the valid
 * part, with
 *   Hs[k] = (1/N) sum_{n<L} h[n] e^{-2 pi i kn/N}
 * computed in double on the host and rounded once to fp32 (the 1/N is a power of two: exact).
 * nsh_fft_filter_tile frames share a workgroup step.
 * Rounding: an output's rounding depends on its frame, and so on how the stream is cut into calls
 * (a call's frames start at its in[0]) -- unlike the direct-form kernels, two chained calls are not
 * bit-identical to one; only hist_out is bit-exact. Within a call a frame's outputs depend on its
 * window alone, bit for bit, whatever follows it, the workgroup that runs it and the grid cap.
 * Accuracy: for output m in frame f, with y_ref the float64 convolution,
 *   |y - y_ref| <= 1e-5 |y_ref| + 1e-6 * max|x over frame f's window| * sum_k |h[k]|
 * Non-finite samples: a non-finite sample makes non-finite every output of every frame whose window
 * holds it (two frames where windows overlap), and touches no other frame.
 * in, out and the histories need only 8-byte alignment.
 * Refused before any HIP call, in this order. nsh_fft_filter_plan_create: a NULL taps_host or plan
 * out-pointer; ntaps outside [1, 4096]; a non-finite tap; an fft_size that is neither 0 nor one of
 * the four sizes; ntaps > fft_size / 2. nsh_fft_filter_ccc: n <= 0 returns 0 and launches nothing,
 * whatever the other arguments; then a NULL in or out; in == out; hist_out aliasing hist_in; a
 * NULL plan; a missing hist_out when ntaps > 1. nsh_fft_filter_grid_cap: a negative cap, then a NULL
 * plan; it bounds the workgroups of the grid-stride walk over the frames (0 restores the default)
 * and the output does not depend on it. An armed nsh_time_next_launch pair is taken by the one
 * launch (dropped when nothing is launched). Runs on the current device, which must be the plan's.
 * Measured: DESIGN.md section 4.8. */
int nsh_fft_filter_plan_create(int dev, const float* taps_host /* ntaps (re, im) pairs */, int ntaps,
                               int fft_size /* 0: chosen by the plan */, void** plan);
int nsh_fft_filter_plan_destroy(void* plan);          /* NULL: 0 */
int nsh_fft_filter_fft_size(void* plan);              /* N; 0 for NULL */
int nsh_fft_filter_valid(void* plan);                 /* V = N - (ntaps - 1); 0 for NULL */
int nsh_fft_filter_history(void* plan);               /* ntaps - 1; 0 for NULL */
int nsh_fft_filter_tile(void* plan);                  /* frames per workgroup step; 0 for NULL */
const char* nsh_fft_filter_kernel(void* plan);        /* e.g. "k_fft_xlat<2048, 1, false>"; "" for NULL */
int nsh_fft_filter_grid_cap(void* plan, int max_workgroups);
int nsh_fft_filter_ccc(void* plan, const float* in, const float* hist_in, float* hist_out, float* out, int64_t n,
                       void* stream);

/* ---- freq_xlating_fft_filter_ccc: tune, filter with complex taps and decimate by overlap-save
 * (GNU Radio's freq_xlating_fft_filter_ccc) ----
 * h = taps_host: ntaps = L complex fp32 taps as (re, im) pairs, 1 <= L <= 4096; D = decim in
 * {1, 2, 4, 8, 16, 32, 64}; inc = nsh_phase_inc(-freq_norm); nsh_fir_xlat_ccf's definition with
 * complex taps:
 *   y[m] = sum_{k<L} h[k] * x[mD-k] * exp(+j 2 pi phase(first_index + mD - k))
 *        = exp(+j 2 pi phase(first_index + mD)) * sum_{k<L} g[k] * x[mD-k]
 *   phase(n) = ((n * inc) mod 2^64) / 2^64 turns,  g[k] = h[k] * exp(-j 2 pi ((k * inc) mod 2^64) / 2^64)
 * The second line is what runs: the band-pass taps g are formed in double on the host from the
 * 64-bit inc, Hs[k] = (1/N) DFT_N(g) is rounded once to fp32, and the remaining rotation is applied
 * to the outputs at the phase ((first_index + m*D) * inc) mod 2^64 in uint64 wrap-around, so an
 * output's phase does not depend on how the stream is cut into calls (its phasor is the rounded
 * product of two: that of the first output its lane holds in the frame and that of the distance from
 * it, each from the top 32 bits of its exact 64-bit phase). With inc == 0 the rotation is skipped,
 * not multiplied by one. A call consumes n_out * D inputs. History as nsh_fir_xlat_ccf (L-1 raw samples,
 * hist_out bit-exact, must not alias hist_in, required when L > 1).
 * Frames: N = fft_size in {1024, 2048, 4096, 8192} with L <= N/2; 0 lets the plan choose by
 * nsh_fft_filter_plan_create's rule. O = L-1 rounded up to a multiple of D (nsh_fft_xlat_overlap),
 * V = N - O (nsh_fft_xlat_valid), Vd = V/D outputs per frame, M = N/D. Frame f of a call owns
 * out[f*Vd, (f+1)*Vd) up to n_out and reads the window of inputs [fV-O, fV-O+N): positions in
 * [-(L-1), 0) come from the history (or are zeros), positions below are zeros (they reach discarded
 * outputs only), positions at or past n_out*D are zeros; nothing at or past out[n_out] is stored.
 * One launch of k_fft_xlat<N, D> per call: window -> forward FFT of N -> times Hs -> fold
 * Z[k'] = Y[k'] + Y[k'+M] + ... + Y[k'+(D-1)M] (in this order) -> unnormalised inverse FFT of M
 * points -> drop the first O/D -> times the phasor -> store. nsh_fft_xlat_tile frames share a
 * workgroup step.
 * Rounding: as nsh_fft_filter_ccc, an output's rounding depends on where its frame starts, so two
 * chained calls agree with one call to the bound below, not bit for bit; the phase and hist_out are
 * exact. Within a call a frame's outputs depend on its window, first_index and its place in the
 * call's frame grid alone, bit for bit, whatever follows it, the workgroup that runs it and the
 * grid cap. D = 1 with freq_norm = 0 is the same kernel as nsh_fft_filter_ccc at the same fft_size
 * (which runs it with the rotation compiled out: the same bits).
 * Accuracy: for output m in frame f, with y_ref the float64 evaluation of the first line,
 *   |y - y_ref| <= 1e-5 |y_ref| + 1e-6 * max|x over frame f's window| * sum_k |h[k]|
 * Non-finite samples: a non-finite sample makes non-finite every output of every frame whose window
 * holds it, and touches no other frame.
 * in, out and the histories need only 8-byte alignment.
 * Refused before any HIP call, in this order. nsh_fft_xlat_plan_create: a NULL taps_host or plan
 * out-pointer; ntaps outside [1, 4096]; a non-finite tap; a decim that is not a power of two in
 * [1, 64] (nsh_fir_xlat_ccf stays the entry point for other decimations); a non-finite freq_norm; an
 * fft_size that is neither 0 nor one of the four sizes; ntaps > fft_size / 2. nsh_fft_xlat_ccc:
 * n_out <= 0 returns 0 and launches nothing, whatever the other arguments; then a NULL in or out;
 * in == out; hist_out aliasing hist_in; a NULL plan; a missing hist_out when ntaps > 1; n_out * D
 * too large for one call. nsh_fft_xlat_grid_cap: a negative cap, then a NULL plan; 0 restores the
 * default, and the output does not depend on it. An armed nsh_time_next_launch pair is taken by the
 * one launch (dropped when nothing is launched). Runs on the current device, which must be the
 * plan's. On a machine with no device at all nsh_fft_xlat_plan_create still makes the plan, so that its
 * geometry can be asked for; its tables stay on the host, and the first nsh_fft_xlat_ccc (which needs
 * a device) would upload them. Measured: DESIGN.md section 4.10. */
int nsh_fft_xlat_plan_create(int dev, const float* taps_host /* ntaps (re, im) pairs */, int ntaps, int decim,
                             double freq_norm, int fft_size /* 0: chosen by the plan */, void** plan);
int nsh_fft_xlat_plan_destroy(void* plan);            /* NULL: 0 */
int nsh_fft_xlat_fft_size(void* plan);                /* N; 0 for NULL */
int nsh_fft_xlat_decim(void* plan);                   /* D; 0 for NULL */
int nsh_fft_xlat_overlap(void* plan);                 /* O; 0 for NULL */
int nsh_fft_xlat_valid(void* plan);                   /* V = N - O; 0 for NULL */
int nsh_fft_xlat_history(void* plan);                 /* ntaps - 1; 0 for NULL */
int nsh_fft_xlat_phase_inc(void* plan, uint64_t* inc); /* NULL plan or inc: refused */
int nsh_fft_xlat_tile(void* plan);                    /* frames per workgroup step; 0 for NULL */
const char* nsh_fft_xlat_kernel(void* plan);          /* e.g. "k_fft_xlat<2048, 8>"; "" for NULL */
int nsh_fft_xlat_grid_cap(void* plan, int max_workgroups);
int nsh_fft_xlat_ccc(void* plan, const float* in, const float* hist_in, float* hist_out, float* out, int64_t n_out,
                     uint64_t first_index, void* stream);

/* ---- psd_vcf: windowed FFT, |X|^2 and the sum over K frames (fft_vcc -> complex_to_mag_squared ->
 * integrate_ff -> nlog10_ff) in one pass over the input ----
 * N = fft_size, a power of two in [16, 8192]; K = navg in [1, 65536]; w = window_host, N floats
 * (host; copied; NULL: none); scale finite and > 0 (1/K for the mean, 1/(K sum w^2) for a density).
 * Output vector j takes the frames f = jK .. jK+K-1 of the input, frame f being samples fN .. fN+N-1
 * (frames do not overlap):
 *   X_f[k]   = sum_n x_f[n] w[n] e^{-2 pi i kn/N}     exactly as a forward nsh_fft_c2c plan with w
 *   P_j[k]   = scale * sum_f |X_f[k]|^2
 *   out_j[k] = P_j[k ^ (shift ? N/2 : 0)],  or 10 * log10f of that value when db is set (a zero sum
 *              gives -inf: the documented result, not an error).
 * nsh_psd_cf reads nvec * K * N complex samples and writes nvec * N floats; in needs 8-byte and out
 * 4-byte alignment; they must not alias. Every sample is read once: 8 + 4/K bytes of HBM traffic per
 * sample while K <= P.
 * The K frames of a vector are cut into nseg = ceil(K / 32) segments of P = ceil(K / nseg) frames
 * (nsh_psd_segment; a plan constant that depends on K alone: K up to 32, 17 at K = 33, 32 at 1024; the
 * last segment may be shorter); a segment's frames are added in order in fp32 registers. With one segment the result is
 * stored at once (one launch of nsh_psd_kernel). With more, the segments' sums go to scratch memory
 * the plan owns and a second small kernel adds each vector's segments in a fixed order; a call with
 * more segments than the scratch holds runs in batches of whole vectors. Because of the scratch a
 * plan serves one stream at a time.
 * Cut invariance: the chain of additions of a vector depends on (N, K, P) alone, so a vector's N
 * outputs are bit-identical whatever the number of vectors in the call, the vector's place in it,
 * the grid cap and the vector's slot in a wave or workgroup (nsh_psd_tile segments share a workgroup
 * step). No float atomics.
 * Non-finite samples: a non-finite sample makes the N outputs of its own vector non-finite and leaves
 * every other vector bit-identical; the same holds for a frame whose |X|^2 overflows fp32.
 * Accuracy: with X_f the float64 transform, d_f = 1e-5 max_k |X_f[k]| and g = (K + 2) 2^-24,
 *   |out_j[k] - P_j[k]| <= scale * [sum_f (2 |X_f[k]| d_f + d_f^2) + g sum_f |X_f[k]|^2]
 * Refused before any HIP call, in this order. nsh_psd_plan_create: a NULL plan out-pointer; an
 * fft_size that is not a power of two in [16, 8192]; navg outside [1, 65536]; a non-finite window
 * entry; a scale that is not finite or not > 0. nsh_psd_cf: nvec <= 0 returns 0 and launches
 * nothing, whatever the other arguments; then a NULL in or out; in == out; a NULL plan; nvec so large
 * that the byte counts overflow. nsh_psd_grid_cap: a negative cap, then a NULL plan; it bounds the
 * workgroups of the grid-stride walk over the segments (0 restores the default) and the output does
 * not depend on it. An armed nsh_time_next_launch pair is taken by the call: its start is recorded
 * with the first launch and its stop with the last (dropped when nothing is launched). Runs on the
 * current device, which must be the plan's.
 * Measured: DESIGN.md section 4.9. */
int nsh_psd_plan_create(int dev, int fft_size, int navg, const float* window_host /* NULL: none */, int shift,
                        float scale, int db, void** plan);
int nsh_psd_plan_destroy(void* plan);                 /* NULL: 0 */
int nsh_psd_fft_size(void* plan);                     /* N; 0 for NULL */
int nsh_psd_navg(void* plan);                         /* K; 0 for NULL */
int nsh_psd_segment(void* plan);                      /* P; 0 for NULL */
int nsh_psd_tile(void* plan);                         /* segments per workgroup step; 0 for NULL */
const char* nsh_psd_kernel(void* plan);               /* e.g. "k_psd<4096, false>"; "" for NULL */
int nsh_psd_grid_cap(void* plan, int max_workgroups); /* 0 restores the default */
int nsh_psd_cf(void* plan, const float* in, float* out, int64_t nvec, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* NSH_HIP_H */
