/*
 * waveverify_hip.h — C ABI of libwaveverify_hip.so: the MI355X (gfx950) embed/detect hot path
 * of WaveVerify.  Plain pointers and sizes only; no torch / HIP types in the signatures
 * (`stream` is a hipStream_t passed as void*, NULL = the default stream).
 *
 * What each entry point replaces in the reference (paths relative to /root/reference):
 *   wv_generator_forward  Generator.forward            model/generator.py:360-423
 *                         (+ the `wm = delta + x` of AudioWatermarking._forward_audio_sample,
 *                          model/watermarking.py:423-441, when add_input != 0, and the message
 *                          batch broadcast of watermarking.py:320-329 through msg_rows)
 *   wv_detector_forward   Detector.forward             model/detector.py:366-391
 *                         (+ sigmoid/mean-over-time of waveverify/core.py:577-580 when
 *                          mean_prob != NULL, so the [B,nbits,T] logits need not be stored)
 *   wv_locator_forward    Locator.forward              model/locator.py:268-299
 *   wv_window_* / wv_session_advance / wv_segment_track / wv_detector_forward_windowed
 *                         not in the reference: windowed long-form and live-session execution
 *   wv_loudness / wv_pool_sample
 *                         the data path of scripts/train.py:440-475 (audiotools' AudioDataset: a random excerpt,
 *                         re-drawn until its BS.1770 loudness exceeds the cutoff), as a restatement of the standard
 *   wv_model_set_param*   nn.Module.load_state_dict on the stripped / parametrized key layouts
 *                         waveverify/core.py:324-426, scripts/train.py:1589-1676
 *   wv_op_*               the fused units of modules/seanet.py + modules/conv.py, exported one by
 *                         one so that parity tests can pin each kernel separately.
 *
 * Tensors are float32, contiguous, [B, C, T] with time innermost, in DEVICE memory unless the
 * parameter is documented as host memory.  The caller owns every buffer; the library owns only
 * the packed weights inside a wv_model.  Every function returns 0 on success or a negative
 * WV_E* code; after a non-zero return wv_last_error() gives the reason (thread-local).
 */
#ifndef WAVEVERIFY_HIP_H
#define WAVEVERIFY_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define WV_OK 0
#define WV_EINVAL (-1)   /* bad argument / shape */
#define WV_ENOKEY (-2)   /* unknown or missing parameter name */
#define WV_EHIP (-3)     /* HIP runtime error */
#define WV_ESTATE (-4)   /* call order (e.g. forward before finalize) */
#define WV_ENOMEM (-5)   /* workspace too small */

#define WV_KIND_GENERATOR 0
#define WV_KIND_DETECTOR 1
#define WV_KIND_LOCATOR 2

#define WV_MAX_STRIDES 8

/* Hyper-parameters; field names follow the reference constructors
 * (model/generator.py:63-104, model/detector.py:82-114, model/locator.py:84-115). */
typedef struct wv_config {
    int32_t kind;
    int32_t dimension;
    int32_t msg_dimension;
    int32_t channels_enc;
    int32_t channels_dec;
    int32_t n_fft_base;
    int32_t n_residual_enc;
    int32_t n_residual_dec;
    int32_t n_strides;
    int32_t strides[WV_MAX_STRIDES];   /* as given to the constructor, e.g. {8,5,4,2} */
    int32_t kernel_size;
    int32_t last_kernel_size;
    int32_t residual_kernel_size;
    int32_t dilation_base;
    int32_t zero_init;                 /* 1: res_scale_param / scale_param tensors exist */
    int32_t nbits;
    int32_t output_dim;
    int32_t embedding_dim;
    int32_t embedding_layers;
    int32_t freq_bands;
    float res_scale_enc;
    float res_scale_dec;
    float wav_std;
    float spec_means[WV_MAX_STRIDES + 1];
    float spec_stds[WV_MAX_STRIDES + 1];
} wv_config;

typedef struct wv_model wv_model;

/* The message of the calling thread's most recent FAILED call.  Like errno it is defined only after a non-zero return: a successful
 * call neither clears nor touches it.  Every non-zero return of every function below stores its reason here. */
const char* wv_last_error(void);
const char* wv_version(void);

/* Fill cfg with the reference defaults for `kind`. */
int wv_config_default(int kind, wv_config* cfg);

/* ==== csrc/wv_model.hip ================================================================== */
/* ---- model lifetime --------------------------------------------------------------------- */
int wv_model_create(const wv_config* cfg, wv_model** out);
void wv_model_destroy(wv_model* m);

/* Parameter table: the state-dict keys (stripped layout) this model expects. */
int wv_model_num_params(const wv_model* m);
/* name_out: caller buffer of name_cap bytes; shape_out: 4 int64 (unused dims = 1). */
int wv_model_param_info(const wv_model* m, int index, char* name_out, int name_cap,
                        int64_t* shape_out, int* ndim_out, int* is_weight_normed);

/* Hand over one tensor in the reference's layout (HOST memory, float32, numel checked). */
int wv_model_set_param(wv_model* m, const char* name, const float* host_data, int64_t numel);
/* Same for a weight-normed tensor given as the (g, v) pair of
 * `...parametrizations.weight.original0/1`; folded as w = g * v / ||v|| (modules/conv.py:73-74). */
int wv_model_set_param_wn(wv_model* m, const char* name, const float* host_g, int64_t g_numel,
                          const float* host_v, int64_t v_numel);
/* Optional override of a CausalSTFT basis buffer `...spec.weight` [2F,1,n_fft] (checkpoints
 * carry it, modules/conv.py:1026); by default the basis is generated as conv.py:1003-1020 does. */
int wv_model_set_stft_basis(wv_model* m, const char* name, const float* host_data, int64_t numel);
/* Pack (transpose / interleave / compose heads) and upload. Fails if a parameter is missing. */
int wv_model_finalize(wv_model* m);

/* ---- forward passes --------------------------------------------------------------------- */
/* Device scratch needed for a [B,1,T] batch (bytes). */
size_t wv_workspace_bytes(const wv_model* m, int B, int T);

/* x [B,1,T]; msg [msg_rows, msg_dimension] float (0/1), msg_rows == B or 1 (broadcast);
 * out [B,1,T] = delta, or delta + x when add_input != 0. */
int wv_generator_forward(wv_model* m, const float* x, const float* msg, int msg_rows,
                         float* out, int add_input, int B, int T,
                         void* workspace, size_t workspace_bytes, void* stream);

/* x [B,1,T]; logits [B,nbits,T] or NULL; mean_prob [B,nbits] or NULL (mean_t sigmoid(logit)). */
int wv_detector_forward(wv_model* m, const float* x, float* logits, float* mean_prob,
                        int B, int T, void* workspace, size_t workspace_bytes, void* stream);

/* x [B,1,T]; logits [B,1,T]. */
int wv_locator_forward(wv_model* m, const float* x, float* logits, int B, int T,
                       void* workspace, size_t workspace_bytes, void* stream);

/* Encoder only (SEANetEncoder.forward, modules/seanet.py:883-976): latent [B,dimension,ceil(T/hop)].
 * msg may be NULL (no FiLM), as for the detector / locator. */
int wv_encoder_forward(wv_model* m, const float* x, const float* msg, int msg_rows, float* latent,
                       int B, int T, void* workspace, size_t workspace_bytes, void* stream);

/* The same three forwards in the f16-operand mode (described with the wv_h16_* units below). */
int wv_detector_forward_f16(wv_model* m, const float* x, float* logits, float* mean_prob,
                            int B, int T, void* workspace, size_t workspace_bytes, void* stream);
int wv_locator_forward_f16(wv_model* m, const float* x, float* logits, int B, int T,
                           void* workspace, size_t workspace_bytes, void* stream);
int wv_generator_forward_f16(wv_model* m, const float* x, const float* msg, int msg_rows,
                             float* out, int add_input, int B, int T,
                             void* workspace, size_t workspace_bytes, void* stream);

/* Localized detection: the detector in its gated per-FRAME form (frame f = samples [f*hop, min((f+1)*hop, T)), Fr = ceil(T/hop)).
 * x [B,1,T]; gate [B,T] f32 DEVICE or NULL; sample t of clip b is gated iff gate == NULL || gate[b][t] > gate_thr (strict, as the
 * reference's locator_out > 0.5).  Locator LOGITS go in as they are with gate_thr = log(p / (1 - p)), a 0/1 mask with gate_thr = 0.5.
 * fsum [B, nbits + 1, Fr] f32: row bit < nbits, frame f = the sum over the gated samples of the frame of sigmoid(logit[bit][t]); row
 * nbits = the number of gated samples of the frame (an exact integer).  Every element is written, zeros included; no logits are stored;
 * the summation order is fixed, so two runs agree bit for bit.  Workspace and routing of wv_detector_forward (_f16: of
 * wv_detector_forward_f16 with logits == NULL; where its f16 head does not apply, the exact frames kernel runs on the f32 tail). */
int wv_detector_forward_frames(wv_model* m, const float* x, const float* gate, float gate_thr, float* fsum,
                               int B, int T, void* workspace, size_t workspace_bytes, void* stream);
int wv_detector_forward_frames_f16(wv_model* m, const float* x, const float* gate, float gate_thr, float* fsum,
                                   int B, int T, void* workspace, size_t workspace_bytes, void* stream);

/* message MLP + all FiLM gammas/betas (seanet.py:831-846,905-912): msg [rows,msg_dim] ->
 * film [B,n_scales,bands,2]; uses the model's parameters. */
int wv_model_film(wv_model* m, const float* msg, int msg_rows, float* film, int B, void* stream);

/* ---- measurement hook (bench.py's roofline figures) ---------------------------------------
 * When enabled, every kernel launch is bracketed by a hipEvent pair on the launch stream and
 * aggregated by "<kernel>|<role>" together with its ALGORITHMIC flops and bytes (the per-unit
 * figures of DESIGN.md).  wv_profile_collect(-1, ...) synchronises, snapshots and returns the
 * number of entries; wv_profile_collect(i, ...) reads entry i of that snapshot. */
int wv_profile_enable(int on);
int wv_profile_reset(void);
int wv_profile_collect(int index, char* name_out, int name_cap, int64_t* launches,
                       double* total_ms, double* flops, double* bytes);

/* ==== csrc/wv_window.hip (the two windowed forwards: csrc/wv_model.hip) ===================== */
/* ---- windowed long-form and live sessions (waveverify_amd/window.py, session.py) -----------
 * A clip or a stream runs as a batch of WINDOWS of L samples: a run of frames plus a left halo no shorter than the net's
 * receptive field (window.halo), window starts and keep edges on hop multiples counted from the clip's t = 0.  The window
 * batch goes through the forwards above; only each window's kept columns are written back.  Sizes are in samples.
 *   wv_window_gather       dst [W,1,L]: window w = src[offs[w] .. offs[w] + L), src the packed clips (n_src samples),
 *                          offs [W] int64 device.  Windows lying outside src are skipped; nothing is zero-filled.
 *   wv_window_scatter      y [W,C,L] -> out (n_out floats): desc [W][4] int64 device = {offset in out of the window's column 0,
 *                          row stride of its clip's [C,T] output, keep lo, keep hi} (keep range relative to the window);
 *                          out[desc0 + c*desc1 + j] = y[w][c][j] for j in [lo, hi).
 *   wv_detector_forward_windowed   x [W,1,L]; keep_lo / keep_hi [W] int32 device (relative to the window); psum [W,nbits] =
 *                          sum over t in [keep_lo, keep_hi) of sigmoid(logit) -- the logits are never stored.  Workspace
 *                          of wv_detector_forward for (W, L); the _f16 twin runs the f16-operand mode.
 *   wv_window_reduce_mean  mean_prob [B,nbits] = (sum over psum rows rows[ptr[b] .. ptr[b+1]) in that order, in f64) / lengths[b];
 *                          ptr [B+1] / rows int32, lengths [B] int64, all device.
 *   wv_frames_reduce       fsum [B, nb + 1, Fr_stride] (wv_detector_forward_frames) -> per segment seg [n_seg][3] int32 device = {clip,
 *                          f_lo, f_hi}: S[bit] and N = the sums over frames f_lo .. f_hi - 1, in that order, in f64, of row bit and of the
 *                          count row; prob [n_seg, nb] f32 = S / (float(N) + eps) (the eps add in f32, as wv_metrics_decode makes it, the
 *                          quotient rounded once), count [n_seg] f64 = N.  N == 0 gives prob = 0: "no watermark found" is the host's
 *                          to report.  A segment reaching outside the tensor counts as empty.  Segments may overlap.
 *   wv_session_advance     one tick of S lockstep sessions: stream s's samples are cat(hist[s][0 .. hv), x[s][0 .. n)) with
 *                          hist [S,hcap], x [S,n]; win [S,1,wlen] = their first wlen samples (wlen may be 0), hist_out [S,hcap] =
 *                          their samples [drop, drop + hv2); drop + hv2 == hv + n, hist_out != hist.
 *   wv_segment_track       the streaming form of localize.segments_from_counts + wv_frames_reduce: one tick of S lockstep segment trackers.
 *                          fsum [S, nb + 1, Fr_stride] as above; this tick's frames are its columns [f_lo, f_hi) (f_hi == f_lo: none), column f_lo
 *                          being the stream's frame number frame0 (the caller counts frames; ticks must follow one another without a gap).
 *                          A frame is ON when valid > 0 and (double)count >= min_on * valid, valid = hop, or last_valid for the last frame of a
 *                          `final` tick.  An on frame opens a run, or extends the open run [lo, hi): the off frames since hi are added first,
 *                          one by one in ascending order, then the frame itself, each as one f64 add per row, which is the order
 *                          wv_frames_reduce takes over [lo, hi).  A run CLOSES once min_gap_frames off frames have followed it, or on `final`;
 *                          a run shorter than min_len_frames is dropped, any other becomes the stream's next event {lo, hi, count = N,
 *                          prob = S / (float(N) + eps), 0 where N == 0} exactly as wv_frames_reduce computes it.  After a final tick the
 *                          stream's state is closed; zero both buffers to start over.  One workgroup per stream, one thread per row; no
 *                          atomics.  Nothing outside state and events is written, and fsum is only read.
 *                          A state that cannot follow from zeros and gapless ticks (lo, hi or the counter out of range for this frame0) is
 *                          taken as closed with no events, so that garbage in the buffers never becomes an address outside them.
 *                          Both buffers are the caller's, 8-byte aligned, all zeros before the first tick, sized by wv_segment_track_bytes:
 *                            state,  per stream (stride 32 + 8 (nb + 1) + roundup8(4 (min_gap_frames - 1)(nb + 1)) bytes):
 *                                    int64 {open 0/1, lo, hi, frames seen}; f64 sum[nb + 1] of the open run's rows over [lo, hi) (row nb = N);
 *                                    f32 ring[min_gap_frames - 1][nb + 1], the raw off frames after hi, frame j in slot j % (min_gap_frames - 1)
 *                            events, per stream (stride 8 + capacity * rec bytes, rec = 24 + roundup8(4 nb)):
 *                                    int64 n = events so far (monotonic); record c: int64 lo, int64 hi, f64 count, f32 prob[nb]; event number e
 *                                    (from 0) is record e % capacity, so a reader that polls before `capacity` events pile up loses none.
 *                          Refused with WV_EINVAL: S outside [1, 65535], nb outside [1, WV_SEGMENT_MAX_BITS], min_gap_frames outside
 *                          [1, WV_SEGMENT_MAX_GAP], capacity < 1, null or short buffers, frames outside the tensor.
 *   wv_bank_advance        one tick of a session BANK (session.py): `capacity` independent streams, of which the P
 *                          named by desc pushed samples this tick.  hist [capacity, hcap] is updated IN PLACE; x (n_x floats) holds the new
 *                          samples of all pushed slots, packed; desc [P][8] int64 device = {slot, hv, x_off, n, row, wlen, drop, hv2}.  The
 *                          stream's samples are cat(hist[slot][0 .. hv), x[x_off .. x_off + n)).  Where wlen > 0, win[row][0 .. wlen) = their
 *                          first wlen samples and win[row][wlen .. Lmax) = 0, win being [A, 1, Lmax]; hist[slot][0 .. hv2) becomes their samples
 *                          [drop, drop + hv2).  hist[slot][hv2 .. hcap) keeps whatever it held and is never read back (the next tick's hv is
 *                          this tick's hv2).  History rows and window rows that desc does not name are not touched, and the launch grows
 *                          with P and Lmax, not with capacity.
 *                          THE CALLER'S DUTY: the slots of one call are distinct, and so are the rows of its windowed descriptors; two rows
 *                          naming one slot would shift one history twice, in no defined order.
 *                          A descriptor row is SKIPPED whole (no window columns, no history change) unless 0 <= slot < capacity,
 *                          0 <= hv <= hcap, 0 <= hv2 <= hcap, n >= 0, drop >= 0, drop + hv2 == hv + n, 0 <= wlen <= min(hv + n, Lmax),
 *                          0 <= x_off and x_off + n <= n_x, and, where wlen > 0, 0 <= row < A; the other rows of the call are served.
 *                          Refused with WV_EINVAL and nothing written: null hist or desc, n_x > 0 without x, A > 0 without win;
 *                          capacity outside [1, WV_BANK_MAX_SLOTS], hcap < 1, n_x < 0, P or A outside [0, 65535], Lmax < 0 (or < 1 with
 *                          A > 0); hist, x and win ranges that overlap.  P == 0 is success without a launch.
 *                          The descriptor carries nothing of a net: a second per-slot history (a segment bank's gate) goes through the
 *                          same call with the same rows.
 *   wv_bank_detect_update  one tick of a detect bank: psum [A, nb] (wv_detector_forward_windowed on the tick's windows), desc [A][2] int64
 *                          device = {slot, samples}.  Per row r and bit k: acc[slot][k] += (double)psum[r][k]; seen[slot] += samples;
 *                          mean_prob[r][k] = (float)(acc[slot][k] / max(seen[slot], 1)); bits[r][k] = mean_prob[r][k] >= 0.5f.  acc
 *                          [capacity, nb] f64 and seen [capacity] int64 are the bank's state, zero for a fresh slot; slots not named are
 *                          untouched; a row whose slot is outside [0, capacity) or whose samples < 0 is skipped.  The slots of one call
 *                          are distinct (the caller's duty).  One thread per (row, bit), no atomics.  A == 0 is success without a launch.
 *   wv_bank_segment_track  one tick of a segment BANK (session.py SegmentBank): `capacity` independent segment trackers,
 *                          of which the P named by desc take frames this tick, each its own range.  state and events hold `capacity` streams
 *                          in exactly wv_segment_track's per-stream layouts (above), sized by wv_segment_track_bytes(capacity, nb,
 *                          min_gap_frames, ring, ...), `ring` being the event records per slot; slot s is stream s of them, so a slot's bytes
 *                          after the same ticks are those wv_segment_track leaves, and the same host readers serve both.  A fresh slot is all
 *                          zeros in both buffers (the caller clears a slot it hands to a new stream).
 *                          fsum is ONE arena of n_fsum floats that holds the frame sums of every launch of the tick, each launch with its
 *                          own row length; desc [P][8] int64 device = {slot, fsum_off, Fr_stride, f_lo, f_hi, frame0, last_valid, final}.
 *                          Row k (k <= nb, row nb the count row) of that stream's sums starts at fsum + fsum_off + k * Fr_stride; this tick's
 *                          frames are its columns [f_lo, f_hi), column f_lo being the stream's frame number frame0 (the caller counts a slot's
 *                          frames; its ticks follow one another without a gap).  final != 0 ends the stream: last_valid counts as the valid
 *                          samples of the last frame of such a row only (any other frame has hop), the open run closes, and f_hi == f_lo
 *                          with final closes it without adding a frame.  A row with f_hi == f_lo that is not final changes nothing.
 *                          Per stream the tick is wv_segment_track's, the same device function: the ON rule, the f64 adds in ascending frame
 *                          order with the gap's off frames first, the gap ring (frame j in slot j % (min_gap_frames - 1)), the close after
 *                          min_gap_frames off frames, the min_len_frames drop, prob = S / (float(N) + eps), and a state that cannot follow
 *                          from zeros and gapless ticks taken as closed with no events.  One workgroup per descriptor, thread k <= nb owns
 *                          row k; no atomics; state is read before one barrier and written after it.  Nothing outside the named slots'
 *                          state and event sections is written, and fsum and desc are only read.
 *                          THE CALLER'S DUTY: the slots of one call are distinct; two rows naming one slot would run one tracker twice at
 *                          once.  The frames of one slot may be split over several calls on the same fsum with sub-ranges of [f_lo, f_hi).
 *                          A descriptor row is SKIPPED whole (its slot untouched) unless 0 <= slot < capacity, 0 <= f_lo <= f_hi <= Fr_stride
 *                          <= 2^31 - 1, 0 <= fsum_off and fsum_off + (nb + 1) * Fr_stride <= n_fsum, frame0 >= 0 and 0 <= last_valid <= hop;
 *                          the other rows of the call are served.
 *                          Refused with WV_EINVAL and nothing written: null desc, state or events, n_fsum < 0 or n_fsum > 0 without fsum;
 *                          capacity outside [1, WV_BANK_MAX_SLOTS], P outside [0, 65535], nb outside [1, WV_SEGMENT_MAX_BITS], hop < 1,
 *                          min_gap_frames outside [1, WV_SEGMENT_MAX_GAP], min_len_frames < 0, ring < 1, min_on not a number; state or
 *                          events shorter than `capacity` streams need, or not 8-byte aligned.  P == 0 is success without a launch.
 *   wv_segment_track_split / wv_bank_segment_track_split
 *                          wv_segment_track and wv_bank_segment_track under a SPLIT RULE (localize.SplitRule is the definition, DESIGN.md
 *                          section 7d-10): runs [lo, hi) are found exactly as there (same ON rule, gap merge, close and min_len_frames drop of
 *                          the whole run), and a run is also cut where the decoded id changes.  With W = window_frames and plo the start of
 *                          the run's current piece (lo at first), a frame boundary g is a CANDIDATE once plo + W <= g and g + W <= hi.  L_k
 *                          and R_k (k = 0 .. nb, row nb the count row) are the sums of row k over frames [g - W, g) and [g, g + W), each f32
 *                          widened to f64 and added one by one in ascending order.  Where L_nb > 0 and R_nb > 0, S(g) = the sum over
 *                          k = 0 .. nb - 1 in ascending k of |L_k / L_nb - R_k / R_nb| and d(g) = the number of k with
 *                          (L_k / L_nb >= 0.5) != (R_k / R_nb >= 0.5); g QUALIFIES when S(g) >= threshold and d(g) >= min_bits.  Candidates
 *                          are evaluated in ascending g as soon as `hi` allows, with at most one pending (cg, cS): first, if one is pending
 *                          and g - cg >= W, cg is committed; then a qualifying g becomes pending if none is or S(g) > cS strictly.  A commit
 *                          emits the piece [plo, cg) and sets plo = cg.  When the run closes, a pending cut is committed without waiting and
 *                          [plo, hi) is emitted.  So every piece has at least W frames, a cut at g is known once frame g + 2 W - 1 has
 *                          arrived, and a run in which no candidate qualifies gives the event wv_segment_track gives, bit for bit.  A piece's
 *                          sums are one ascending f64 pass over its own frames, prob = S / (float(N) + eps) as above.  No value depends on
 *                          an fma contraction.  One workgroup per stream or descriptor row, thread k <= nb owns row k; the bit terms and
 *                          votes go through LDS and are added in ascending k alike by every thread; no atomics; state is read before the
 *                          last barrier and written after it; fsum (and desc) are only read.
 *                          Buffers as for wv_segment_track, sized by wv_segment_split_bytes(S or capacity, nb, min_gap_frames,
 *                          window_frames, capacity or ring), all zeros for a fresh stream:
 *                            state,  per stream (stride 64 + 8 (nb + 1) + roundup8(4 (2 W + min_gap_frames)(nb + 1)) bytes):
 *                                    int64 {open 0/1, lo, hi, frames seen, plo, pending 0/1, cg}; f64 cS; f64 sum[nb + 1] of the current piece
 *                                    over [plo, sb), sb = max(plo, hi - 2 W + 1); f32 ring[2 W + min_gap_frames][nb + 1], the raw columns of
 *                                    the frames from sb on (the off frames after hi among them), split frame j in slot j % (2 W + min_gap_frames)
 *                            events, per stream (stride 8 + capacity * rec bytes, rec = 32 + roundup8(4 nb)):
 *                                    int64 n = events so far; record c: int64 lo, int64 hi, f64 count, int64 flags (bit 0: the piece's start is
 *                                    an id change, bit 1: its end is one; neither: a locator edge), f32 prob[nb]; event e is record e % capacity.
 *                          A state that cannot follow from zeros and gapless ticks is taken as closed with no events and never becomes an
 *                          address.  As for wv_segment_track, gapless ticks are THE CALLER'S DUTY: frame0 is not compared with the stored
 *                          "frames seen", so a tick that skips or repeats frames while a run is open (possible only within the
 *                          min_gap_frames of slack the check leaves) reads ring columns of other frames: values, never addresses, and
 *                          sums that are then undefined.  The bank form skips bad descriptor rows whole by wv_bank_segment_track's predicate and serves the others.
 *                          Refused with WV_EINVAL and nothing written: everything wv_segment_track / wv_bank_segment_track refuse, and
 *                          window_frames outside [max(2, min_gap_frames, min_len_frames), WV_SPLIT_MAX_WINDOW], threshold not above 0,
 *                          min_bits outside [1, nb].  P == 0 (and a tick without frames that is not final) is success without a launch.
 *   wv_span_gather         span embedding (window.py plan_spans / span_generator): dst [A,1,Lmax] from the packed clips
 *                          src (n_src samples); desc [A][2] int64 device = {src offset, wlen}.  Row r = src[off .. off + wlen), then zeros in
 *                          [wlen, Lmax): a left-aligned, right-zero-padded window batch of rows of their own lengths.  16-byte moves where
 *                          source and destination are aligned, scalar at the edges.
 *                          A descriptor row is SKIPPED whole (its dst row untouched) unless 0 <= off, off + wlen <= n_src and
 *                          0 <= wlen <= Lmax; the other rows are served.
 *                          Refused with WV_EINVAL and nothing written: null desc or dst, n_src < 0 or n_src > 0 without src, A outside
 *                          [0, 65535], Lmax < 1.  A == 0 is success without a launch.
 *   wv_span_scatter_add    y [A,1,Lmax] (the generator's residual on wv_span_gather's batch); desc [A][5] int64 device = {offset in out of the
 *                          window's column 0, keep lo, keep hi, span start, span end}, the last four relative to the window's column 0 (the span
 *                          start may be negative and the span end beyond Lmax: a span spread over several windows).  For j in [lo, hi):
 *                            w = gain * ramp[m] where m = min(j - span start, span end - 1 - j) < F, else w = gain;
 *                            v = w * y[r][j];   out[o + j] = x[o + j] + v   (v alone where x is null)
 *                          all in f32, every rounding kept, no contraction to an fma.  ramp [F] f32 device, null when F == 0.  x may be out
 *                          (each element is read and then written by the same thread); x and out are n_out floats.  Nothing outside the
 *                          rows' keep ranges is written.  THE CALLER'S DUTY: the keep ranges of one call are disjoint in out.
 *                          A descriptor row is SKIPPED whole unless 0 <= lo < hi <= Lmax, span start <= lo, hi <= span end, 0 <= o + lo and
 *                          o + hi <= n_out; the other rows are served.
 *                          Refused with WV_EINVAL and nothing written: null y, desc or out, n_out < 1, F < 0, F > 0 without ramp, gain not a
 *                          number, A outside [0, 65535], Lmax < 1.  A == 0 is success without a launch.
 *   wv_snr_floor           the SNR floor of embedding (snr_floor.py; csrc/wv_snr_floor.hip): x (n_x floats) holds 16 kHz
 *                          model input, r (n_r floats) the generator's residual for it, out (n_out floats) takes the result.  desc [A][8] int64
 *                          device = {offset of the row in x, in r, in out, n, the strength s as its f32 bits (0 .. 2^32 - 1), index into gstate
 *                          or -1, fresh flag, offset in gains or -1}.  ramp [L] f32 device = float32((k + 1) / L); rho = 10^(-min_snr_db / 10).
 *                          Per row, frames of L samples counted from the row's sample 0 (a short last frame only at a stream's true end):
 *                            Ex = sum x^2, Er = sum r^2 in float64, in THE fixed order: sample k of the frame goes to partial (k >> 2) & 15,
 *                              each partial adds in ascending k from +0.0, then p[j] += p[j ^ 8], ^ 4, ^ 2, ^ 1;
 *                            g[f] = s where Er == 0, else q < (double)s ? (float)q : s with q = sqrt((rho * Ex) / Er), divide and square
 *                              root correctly rounded;  g_prev = g[f - 1], for frame 0 gstate[index] or, with index -1 or the fresh flag
 *                              set (the stored value is then not read), g[0];
 *                            w[k] = g_prev < g[f] ? min(g[f], g_prev + (g[f] - g_prev) * ramp[k]) : g[f]     f32, every rounding kept;
 *                            v = w * r;  add == 0: out = v;  add == 1: out = x + v, but x's own bits where v is +0 or -0.
 *                          gstate[index] = the row's last g (a row of n == 0 leaves it alone); gains[offset + f] = g[f].  n_max bounds every
 *                          row's n and sizes the grid.  One launch; the result does not depend on the tile size, the geometry or the row's
 *                          place in the call.  THE CALLER'S DUTY: two rows of one call never name the same state, rows' ranges in out and
 *                          gains are disjoint, and gstate / gains overlap no other argument.
 *                          A descriptor row is SKIPPED whole unless 0 <= n <= n_max, its three ranges lie inside n_x, n_r and n_out, s is
 *                          finite and >= 0, -1 <= index < n_state, and the gains offset is -1 or offset + ceil(n / L) <= n_gains; the other
 *                          rows are served.
 *                          Refused with WV_EINVAL and nothing written: null x, r, out, desc or ramp; a negative size; n_state > 0 without
 *                          gstate or n_gains > 0 without gains; L outside [1, WV_SNR_FLOOR_MAX_FRAME]; rho not finite or <= 0; A outside
 *                          [0, 65535]; n_max outside [0, 2^31 - 1]; add not 0 or 1; out overlapping x or r (a tile reads the frame before
 *                          it again).  A == 0 or n_max == 0 is success without a launch. */
#define WV_SEGMENT_MAX_GAP 64
#define WV_SEGMENT_MAX_BITS 255
#define WV_BANK_MAX_SLOTS 1048576
#define WV_SPLIT_MAX_WINDOW 256
#define WV_SNR_FLOOR_MAX_FRAME 1048576
int wv_window_gather(const float* src, int64_t n_src, const int64_t* offs, float* dst, int W, int L, void* stream);
int wv_window_scatter(const float* y, const int64_t* desc, float* out, int64_t n_out, int W, int C, int L, void* stream);
int wv_detector_forward_windowed(wv_model* m, const float* x, const int* keep_lo, const int* keep_hi, float* psum,
                                 int W, int L, void* workspace, size_t workspace_bytes, void* stream);
int wv_detector_forward_windowed_f16(wv_model* m, const float* x, const int* keep_lo, const int* keep_hi, float* psum,
                                     int W, int L, void* workspace, size_t workspace_bytes, void* stream);
int wv_window_reduce_mean(const float* psum, int n_rows, const int* ptr, const int* rows, const int64_t* lengths,
                          float* mean_prob, int B, int nb, void* stream);
int wv_frames_reduce(const float* fsum, int B, int nb, int Fr_stride, const int* seg, int n_seg, float eps, float* prob, double* count,
                     void* stream);
int wv_session_advance(const float* hist, int hcap, int hv, const float* x, int n, float* win, int wlen,
                       float* hist_out, int drop, int hv2, int S, void* stream);
int wv_segment_track_bytes(int S, int nb, int min_gap_frames, int capacity, size_t* state_bytes, size_t* event_bytes);
int wv_segment_track(const float* fsum, int S, int nb, int Fr_stride, int f_lo, int f_hi, int64_t frame0, int hop, int last_valid,
                     int final, double min_on, int min_gap_frames, int min_len_frames, float eps, void* state, size_t state_bytes,
                     void* events, size_t event_bytes, int capacity, void* stream);
int wv_bank_advance(float* hist, int capacity, int hcap, const float* x, int64_t n_x, const int64_t* desc, int P, float* win, int A,
                    int Lmax, void* stream);
int wv_bank_detect_update(double* acc, int64_t* seen, int capacity, int nb, const float* psum, const int64_t* desc, int A,
                          float* mean_prob, int* bits, void* stream);
int wv_bank_segment_track(const float* fsum, int64_t n_fsum, const int64_t* desc, int P, int capacity, int nb, int hop, double min_on,
                          int min_gap_frames, int min_len_frames, float eps, void* state, size_t state_bytes, void* events, size_t event_bytes,
                          int ring, void* stream);
int wv_segment_split_bytes(int S, int nb, int min_gap_frames, int window_frames, int capacity, size_t* state_bytes, size_t* event_bytes);
int wv_segment_track_split(const float* fsum, int S, int nb, int Fr_stride, int f_lo, int f_hi, int64_t frame0, int hop, int last_valid,
                           int final, double min_on, int min_gap_frames, int min_len_frames, float eps, int window_frames, double threshold,
                           int min_bits, void* state, size_t state_bytes, void* events, size_t event_bytes, int capacity, void* stream);
int wv_bank_segment_track_split(const float* fsum, int64_t n_fsum, const int64_t* desc, int P, int capacity, int nb, int hop, double min_on,
                                int min_gap_frames, int min_len_frames, float eps, int window_frames, double threshold, int min_bits,
                                void* state, size_t state_bytes, void* events, size_t event_bytes, int ring, void* stream);
int wv_span_gather(const float* src, int64_t n_src, const int64_t* desc, float* dst, int A, int Lmax, void* stream);
int wv_span_scatter_add(const float* y, const float* x, const int64_t* desc, const float* ramp, int F, float gain, float* out, int64_t n_out,
                        int A, int Lmax, void* stream);
int wv_snr_floor(const float* x, int64_t n_x, const float* r, int64_t n_r, float* out, int64_t n_out, const int64_t* desc, int A, int64_t n_max,
                 float* gstate, int n_state, float* gains, int64_t n_gains, const float* ramp, int L, double rho, int add, void* stream);

/* ==== csrc/wv_ops.hip ===================================================================== */
/* ---- single fused units ----------------------------------------------------------------
 * Activations (X, resid, film, Y, wav, P, H, x, Z, logits, mean_prob) are DEVICE pointers.
 * Weights / biases (w_*, *_bias, bias, basis) are HOST pointers in the reference's own layouts;
 * they are packed and uploaded per call and the call is synchronous: these entry points exist so
 * that every kernel can be parity-tested on its own, not for serving. */

/* Y = epilogue( DWconv_k,s,d( W1x1 @ act(pre_scale * X) ) + dw_bias )
 *   X [B,K,Tin], w_pw [M,K] (1x1, no bias), w_dw [M,ks], dw_bias [M] or NULL
 *   causal left pad (ks-1)*d-(s-1), zero right pad to complete the last frame
 *   (SConv1d, modules/conv.py:715-763); Tout = ceil(Tin/s).
 *   pre_elu: 1 -> act = ELU, 0 -> identity.
 *   film [B,bands,2] (gamma,beta) or NULL: y = y*gamma+beta per band (seanet.py:928-966);
 *   resid [B,M,Tout] or NULL: y = y*out_scale + resid (seanet.py:272-277).
 * This is the ResnetBlock half (seanet.py:39-116) and the Downsample+FiLM unit (seanet.py:733-772).
 * Yact [B,M,Tout] or NULL: second output ELU(act_scale * y) -- the NEXT unit's prologue hoisted into
 *   this epilogue, so that the consumer can stage its operand by LDS-DMA (a pure copy, pre_elu = 0).
 *   Y may be NULL when only Yact is wanted. */
int wv_op_pw_dw(const float* X, const float* w_pw, const float* w_dw, const float* dw_bias,
                const float* film, const float* resid, float* Y,
                int B, int K, int M, int Tin, int ks, int stride, int dilation,
                float pre_scale, int pre_elu, float out_scale, int bands,
                float* Yact, float act_scale, void* stream);

/* Whole SEANetResnetBlock in one launch, raw in / raw out (narrow layers, C in {64, 96, 128, 192}, k = 5,
 * dilation 1, T % 4 == 0; modules/seanet.py:245-281 with dws_conv_block :39-116):
 *   y = X + out_scale * ( DW5( W2 @ ELU( DW5( W1 @ ELU(pre_scale * X) ) + b1 ) ) + b2 )
 * X [B,C,T] is read once from HBM (activated inside, re-read from L2 as the residual operand); the intermediate
 * stays in LDS.  w_pw1/w_pw2 [C,C]; w_dw1/w_dw2 [C,5]; b1/b2 [C]; Y and/or Yact = ELU(act_scale*y) [B,C,T].
 * Bit-identical to the block run as two wv_op_pw_dw units.
 * Returns WV_EINVAL for shapes the fused kernel does not cover (the nets then run two wv_op_pw_dw units). */
int wv_op_resblock(const float* X, float pre_scale, const float* w_pw1, const float* w_dw1, const float* b1,
                   const float* w_pw2, const float* w_dw2, const float* b2, float* Y, float* Yact,
                   int B, int C, int T, float out_scale, float act_scale, void* stream);

/* Y = W1x1 @ producer(X) + bias, then optional L2-normalise over channels * sqrt(M).
 *   mode 0: producer = act(pre_scale*X)                                  (plain 1x1)
 *   mode 1: producer = causal DW conv k (no bias) of act(pre_scale*X)    (conv_post, seanet.py:797-823)
 *   mode 2: producer = causal DW ConvTranspose k=2r,s=r of act(pre_scale*X), right-trimmed by r
 *           (upsample, seanet.py:1112-1138; SConvTranspose1d conv.py:838-881); Tout = Tin*r
 *   accumulate != 0: Y += out_scale * (W @ producer(X))  (SpecBlock add, seanet.py:500-505).
 * Routing mirrors the model's: mode 2 and the accumulate form with M >= 128 run on the pw_dw kernel
 * (ConvTranspose producer in its operand loader / identity stencil with Y as the residual operand).
 * Yact / act_scale: as for wv_op_pw_dw (mode 2 and the accumulate form with M >= 128 only, else NULL). */
int wv_op_dw_pw(const float* X, const float* w_dw, const float* w_pw, const float* bias, float* Y,
                int B, int K, int M, int Tin, int mode, int ks_or_ratio,
                float pre_scale, int pre_elu, int l2norm, int accumulate, float out_scale,
                float* Yact, float act_scale, void* stream);

/* P[b,f,t] = (log(max(|STFT|,1e-5)) - mean)/std, CausalSTFT magnitude with eps 1e-12
 * (modules/conv.py:1036-1080, seanet.py:479-494). wav [B,1,T]; basis [2F,n_fft] host or NULL
 * (NULL: generated); P [B,F,ceil(T/hop)]. */
int wv_op_stft_logmag(const float* wav, const float* host_basis, float* P, int B, int T,
                      int n_fft, int hop, float mean, float std, void* stream);

/* Whole SpecBlock in one launch (modules/seanet.py:463-511 with CausalSTFT modules/conv.py:1036-1086):
 *   y = x + out_scale * ( W @ P ),  P = (log(max(|STFT(wav)|, 1e-5)) - mean) / std  -- the spectrogram stays in LDS, never in HBM.
 * For the scales whose whole spectrum is one tile and whose 1x1 has as many rows: n_fft = M in {64, 128}, more than 64 frames,
 * Tf = ceil(T/hop) a multiple of 4.  wav [B,1,T]; w_pw [M, n_fft/2+1] (HOST pointer, like every wv_op_* weight); x [B,M,Tf];
 * Y (may alias x) and/or Yact = ELU(act_scale * y).  Bit-identical to wv_op_stft_logmag followed by the accumulate form of wv_op_dw_pw.
 * Returns WV_EINVAL for shapes the fused kernel does not cover (the nets then run the two kernels). */
int wv_op_spec_block(const float* wav, const float* basis_or_null, const float* w_pw, const float* x, float* Y, float* Yact, int B, int T,
                     int n_fft, int hop, int M, float mean, float std, float out_scale, float act_scale, void* stream);

/* conv_pre: Y = Conv1d(1->C,k)(x * in_scale) + bias  (seanet.py:657-664). x [B,1,T], w [C,1,k]. */
int wv_op_conv_pre(const float* x, const float* w, const float* bias, float* Y, int B, int C,
                   int T, int ks, float in_scale, void* stream);

/* decoder tail: out = tanh(out_scale*(Conv1d(C->1,k)(ELU(pre_scale*H)) + bias)) (+ x)
 * (seanet.py:1177-1202, generator.py:410, watermarking.py:440). H [B,C,Tin>=T], w [1,C,k]. */
int wv_op_tail(const float* H, const float* w, const float* bias, const float* x_or_null,
               float* out, int B, int C, int Tin, int T, int ks, float pre_scale, float out_scale,
               void* stream);

/* detector / locator head: ConvTranspose1d(D->O,k=s=hop)+bias -> trim to T -> Conv1d(O->nb,1)+bias
 * (detector.py:300-310). Z [B,D,Fr]; w_rev [D,O,hop]; w_last [nb,O]; either output may be NULL. */
int wv_op_head(const float* Z, const float* w_rev, const float* b_rev,
               const float* w_last, const float* b_last, float* logits, float* mean_prob,
               int B, int D, int O, int nb, int hop, int Fr, int T, void* stream);

/* the same head in the gated per-frame form of wv_detector_forward_frames: gate [B,T] DEVICE or NULL, fsum [B, nb + 1, Fr] DEVICE;
 * Fr must be ceil(T / hop). */
int wv_op_head_frames(const float* Z, const float* w_rev, const float* b_rev, const float* w_last, const float* b_last,
                      const float* gate, float gate_thr, float* fsum, int B, int D, int O, int nb, int hop, int Fr, int T, void* stream);

/* ---- f16-operand / f32-accumulate mode (BASELINE.json configs[4] "MFMA linears fp16"; csrc/wv_h16.hip): a throughput mode of the
 * detector next to the exact-f32 path.  Activations are f16 in the "c8" layout [B][roundup(C,16)/8][T][8] (channel groups of eight,
 * time-major inside a group = the B operand of v_mfma_f32_32x32x16_f16 as it lies in memory); accumulation, stencils, ELU, bias and
 * residual adds are f32.  Weights: HOST f32 pointers in the reference's layouts, as for every wv_op_*.
 *   wv_h16_from_f32 / wv_h16_to_f32   [B,C,T] f32 <-> c8 f16 (from: optionally ELU(scale * x) on the way; rows past C are zero)
 *   wv_h16_conv_pre   conv_pre (seanet.py:657-664) writing c8 f16
 *   wv_h16_resblock   whole SEANetResnetBlock (seanet.py:245-281), C in {32,64,96,128,192,256,384,512,768}, k = 5, dilation 1, any T
 *   wv_h16_conv       y = out_scale * (bias + Conv1d(x)) + resid with W[m][i][k] = w_dw[m][i] * w_pw[m][k] (w_dw NULL: 1), causal,
 *                     x = 0 outside [0,Tin), Tout = ceil(Tin/stride): the downsample unit (ks = 2r, stride r, pad r; seanet.py:739-760)
 *                     and the SpecBlock's 1x1 + add (ks = 1; seanet.py:500-502).  Outputs: Y16 / Yact16 = ELU(act_scale*y) in c8 f16,
 *                     Yf32 [B,M,Tout] f32 row-major (any of them NULL).
 *   wv_h16_spec_block whole SpecBlock in one launch (seanet.py:463-511): the STFT on the f16 pipe with the waveform split in two f16 terms,
 *                     log-magnitude, the 1x1 and the add; the spectrogram stays in LDS.  Every row of the basis is applied (sin_0 and
 *                     sin_{F-1} in f32 beside the matrix product).  (n_fft, hop, M) a row of WV_SPEC16_ROWS (csrc/wv_kernels.h):
 *                     (64,1),(128,2),(256,8),(512,40),(1024,320) with M = n_fft (generator / detector scales), (64,1),(128,4),(256,32)
 *                     with M = n_fft / 2 (the locator's), else WV_EINVAL; x16 / Y16 / Yact16 c8 f16 [B, M/8, ceil(T/hop), 8]
 *   The three forwards below walk a plan that wv_model_finalize decides once from the coverage predicates of csrc/wv_kernels.h: a plan
 *   exists when k = 5, dilation 1, every encoder stage is whole 8-channel groups and its ResnetBlocks an rh16_width (else WV_ESTATE);
 *   a SpecBlock / spec_post runs in one launch where spec16_scale holds (a row of WV_SPEC16_ROWS; spec_post: one marked `post`), else,
 *   or when the launcher refuses a limit of the call, as the exact STFT kernel + the 1x1 on the f16 pipe.
 *   wv_detector_forward_f16   Detector.forward (model/detector.py:366-391) in this mode: conv_pre, the ResnetBlocks, the SpecBlocks
 *                     (STFT as a split-f16 matrix product) incl. spec_post and the downsample units on the f16 pipe; with logits == NULL
 *                     (mean probabilities only) and head16_covers(dimension, nbits, hop) conv_post and the head as well, otherwise
 *                     those two by the exact path's f32 kernels.  Same arguments and workspace as wv_detector_forward.
 *   wv_locator_forward_f16    Locator.forward (model/locator.py:268-299) in this mode: the encoder stages on the f16 pipe (32- and
 *                     64-channel ResnetBlocks, composed downsample convs).  Its SpecBlocks (n_fft = 2 C at every scale) and spec_post
 *                     (256 points, hop 32, 128 channels) each run as ONE fused launch on the f16 pipe: the STFT as a split-f16
 *                     matrix product, NOT the exact path's f32 STFT kernel, with the basis rows sin_0 and sin_{F-1} applied in f32
 *                     beside it; a scale outside WV_SPEC16_ROWS runs the exact STFT kernel + the 1x1 on the f16 pipe.  conv_post
 *                     and the head run on the exact f32 kernels (the locator always returns logits).  Arguments of wv_locator_forward.
 *   wv_generator_forward_f16  Generator.forward (model/generator.py:360-423; modules/seanet.py:883-976, 1067-1226) in this mode: the
 *                     encoder as above with FiLM in the downsample convs' epilogues, conv_post as one composed conv, L2Norm, then
 *                     the decoder: first conv pair as one composed conv, every upsample unit (ELU -> depth-wise ConvTranspose1d ->
 *                     1x1, seanet.py:1147-1170) as ONE two-tap conv over (phase, channel) rows, ResnetBlocks of 768 / 384 / 192 / 96
 *                     channels in one launch each, the tail (f32 sums, tanh, + x) on the c8 stream.  Message MLP / FiLM scalars in f32.
 *                     Arguments and workspace of wv_generator_forward; WV_ESTATE also without a decoder plan (dimension % 16 == 0,
 *                     tail16_taps(last_kernel_size), stages of whole 16-channel group pairs and, with ResnetBlocks, an rh16_width);
 *                     B <= 65535 (the tail's launch grid, wv_h16_tail's limit too).
 *   wv_h16_upsample   the decoder's upsample unit as that conv: x16 = the PRE-ACTIVATED input c8 [B, K/8, Tin, 8]; w_ct [K,1,2r], w_pw
 *                     [M,K,1], bias [M] HOST; Y16 / Yact16 c8 [B, M/8, Tin*r, 8] (either may be NULL)
 *   wv_h16_tail       decoder tail on the pre-activated c8 stream: out[B,1,T] = tanh(out_scale * (b + Conv1d(C -> 1, ks)(a16))) (+ x)
 *   wv_h16_l2norm     L2Norm over channels of lat [B,D,Fr] f32 (seanet.py:288-318) -> c8 f16
 *   wv_h16_head       the mean-probability head of wv_detector_forward_f16 in one launch: L2Norm of lat [B,D,Fr] f32, z as f16, the
 *                     composed head GEMM against f16(wc) (wc [D][nb*hop] HOST, column bit*hop + j; bc [nb] HOST: the exact path's
 *                     ConvTranspose1d(k = s = hop) -> Conv1d(O -> nb, 1) composition), sigmoid, and over t < T (t = frame*hop + j) either
 *                     mean_prob [B,nb] = the mean, or -- keep_lo / keep_hi [B] int32 DEVICE, psum [B,nb] -- psum = the sum over
 *                     t in [keep_lo[b], keep_hi[b]) (mean_prob NULL).  Fr = ceil(T / hop); head16_covers: D % 16 == 0, D <= 128,
 *                     nb % 4 == 0, nb <= 32, hop % 32 == 0, else WV_EINVAL
 *   wv_h16_head_frames  wv_h16_head in the gated per-frame form of wv_detector_forward_frames_f16: gate [B,T] DEVICE or NULL, fsum
 *                     [B, nb + 1, Fr] DEVICE; a frame's sum is taken by the lane that owns it plus one cross-half add.  wv_h16_head's
 *                     limits and hop <= 2016, else WV_EINVAL
 *   wv_h16_conv_film  wv_h16_conv with FiLM behind it (film [B, bands, 2] DEVICE: gamma, beta per clip and band of M / bands rows) */
int wv_h16_round_host(const float* in, uint16_t* out, int64_t n);   /* HOST pointers: the weight packers' f32 -> f16 rounding (nearest even) */
int wv_h16_from_f32(const float* X, void* Y16, int B, int C, int T, float scale, int elu, void* stream);
int wv_h16_to_f32(const void* X16, float* Y, int B, int C, int T, void* stream);
int wv_h16_conv_pre(const float* x, const float* w, const float* bias, void* Y16, int B, int C, int T, int ks, float in_scale, void* stream);
int wv_h16_resblock(const void* X16, float pre_scale, const float* w_pw1, const float* w_dw1, const float* b1, const float* w_pw2, const float* w_dw2,
                    const float* b2, void* Y16, void* Yact16, int B, int C, int T, float out_scale, float act_scale, void* stream);
int wv_h16_conv(const void* X16, const float* w_pw, const float* w_dw, const float* bias, const void* resid16, void* Y16, void* Yact16, float* Yf32,
                int B, int K, int M, int Tin, int ks, int stride, int pad, float out_scale, float act_scale, void* stream);
int wv_h16_spec_block(const float* wav, const float* basis_or_null, const float* w_pw, const void* x16, void* Y16, void* Yact16, int B, int T,
                      int n_fft, int hop, int M, float mean, float std, float out_scale, float act_scale, void* stream);
int wv_h16_upsample(const void* X16, const float* w_ct, const float* w_pw, const float* bias, void* Y16, void* Yact16,
                    int B, int K, int M, int Tin, int ratio, float act_scale, void* stream);
int wv_h16_tail(const void* A16, const float* w, const float* bias, const float* x, float* out, int B, int C, int Tin, int T, int ks,
                float out_scale, void* stream);
int wv_h16_l2norm(const float* lat, void* Y16, int B, int D, int Fr, void* stream);
int wv_h16_head(const float* lat, const float* wc, const float* bc, float* mean_prob, int B, int D, int nb, int hop, int Fr, int T,
                const int* keep_lo, const int* keep_hi, float* psum, void* stream);
int wv_h16_head_frames(const float* lat, const float* wc, const float* bc, const float* gate, float gate_thr, float* fsum, int B, int D, int nb,
                       int hop, int Fr, int T, void* stream);
int wv_h16_conv_film(const void* X16, const float* w_pw, const float* w_dw, const float* bias, const float* film, int bands, void* Y16, void* Yact16,
                     int B, int K, int M, int Tin, int ks, int stride, int pad, float act_scale, void* stream);

/* The same op with the basis packed and uploaded ONCE (a training step computes these features for every scale at every step):
 * basis_or_null as in wv_op_stft_logmag (NULL = the reference's windowed DFT basis). */
typedef struct wv_stft_plan wv_stft_plan;
int wv_stft_plan_create(int n_fft, const float* basis_or_null, wv_stft_plan** out);
void wv_stft_plan_destroy(wv_stft_plan* p);
int wv_stft_plan_logmag(const wv_stft_plan* p, const float* wav, float* P, int B, int T, int hop, float mean, float std, void* stream);
/* backward of the features towards the audio: dwav[B,1,T] (+)= d/dwav of <dP, P(wav)> (training the generator through the detector's and
 * locator's spectrogram branches).  The clamps of the reference (conv.py:1078, seanet.py:484) pass no gradient where |STFT|^2 <= 1e-10. */
size_t wv_stft_plan_backward_workspace_bytes(const wv_stft_plan* p, int B, int T, int hop);
int wv_stft_plan_backward(const wv_stft_plan* p, const float* wav, const float* dP, float* dwav, int accumulate, int B, int T, int hop, float std,
                          void* workspace, size_t workspace_bytes, void* stream);
/* gradient of <dP, P(wav)> towards the BASIS itself (training a generator whose `spec.weight` tensors are nn.Parameters: SEANetEncoder(spec_learnable=True),
 * modules/seanet.py:721,787, modules/conv.py:1023-1024): with C = Basis @ frames(wav), p = re^2 + im^2 and
 * dC = dP * {re, im} / (std * p) where p > 1e-10 (else 0, the same clamp rule as above),
 *     dBasis[m][n] = sum over clips b and frames t of dC[b][m][t] * frames[b][n][t]      ([2F, n_fft] device, overwritten)
 * for all 2F rows (cos_0 .. cos_{F-1}, sin_0 .. sin_{F-1}).  Independent of wv_stft_plan_backward; the sum runs on the training step's
 * time-contracting GEMM with a split plan that depends on the shapes only, so the result repeats bit for bit. */
size_t wv_stft_plan_basis_grad_workspace_bytes(const wv_stft_plan* p, int B, int T, int hop);
int wv_stft_plan_basis_grad(const wv_stft_plan* p, const float* wav, const float* dP, float* dBasis, int B, int T, int hop, float std,
                            void* workspace, size_t workspace_bytes, void* stream);
/* Replace the plan's basis by a DEVICE-resident one ([2F, n_fft], e.g. the parameter an optimizer has just stepped) without a host round
 * trip: every pack of the plan is rewritten by one kernel on `stream`.  The plan then computes exactly what a plan created from the same
 * values would. */
int wv_stft_plan_set_basis_device(wv_stft_plan* p, const float* dev_basis, void* stream);

/* ==== csrc/wv_specloss.hip ================================================================ */
/* Multi-scale STFT and mel-spectrogram reconstruction losses with their gradient towards wm (waveverify_amd/spectral_loss.py holds
 * the semantics).  A plan holds n_scales <= 16 scales; scale i has window length window_lengths[i] (a multiple of 4, >= 8), hop w/4,
 * F = w/2 + 1 bins, and flags[i]: bit 0 = an STFT-magnitude term, bit 1 = a mel term with n_mels[i] bands.  params[8 i .. 8 i + 7] =
 * the STFT term's (log_weight, mag_weight, pow, clamp_eps), then the mel term's.  HOST arrays: windows = the scales' analysis windows
 * concatenated (w floats each); mel_filters = the mel scales' dense [n_mels][F] filters concatenated (scales without a mel term add
 * nothing).  Each term is log_weight * mean|pow log10(max(S_wm, eps)) - pow log10(max(S_x, eps))| + mag_weight * mean|S_wm - S_x| over
 * [B, bins or bands, T/hop + 1] of the centred, reflect-padded transform's magnitude S (or its mel projection). */
typedef struct wv_specloss_plan wv_specloss_plan;
int wv_specloss_plan_create(int n_scales, const int* window_lengths, const int* flags, const int* n_mels, const float* params,
                            const float* windows, const float* mel_filters, wv_specloss_plan** out);
void wv_specloss_plan_destroy(wv_specloss_plan* p);
size_t wv_specloss_workspace_bytes(const wv_specloss_plan* p, int B, int T);
/* wm, x [B,1,T] DEVICE; terms [n_scales][2] (STFT term, mel term; 0 where a scale has none) and totals [2] (sum of the STFT terms, sum
 * of the mel terms) DEVICE float outputs.  dwm [B,1,T] or NULL: dwm += stft_grad_scale * d(STFT total)/dwm + mel_grad_scale *
 * d(mel total)/dwm.  Deterministic (fixed-order sums, no atomics).  WV_EINVAL when T <= w/2 for some scale (reflect padding). */
int wv_specloss(const wv_specloss_plan* p, const float* wm, const float* x, int B, int T, float* terms, float* totals, float* dwm,
                float stft_grad_scale, float mel_grad_scale, void* workspace, size_t workspace_bytes, void* stream);

/* ==== csrc/wv_train.hip: the training step =======================================================
 * Forward and backward of the nets' fused units with LIVE weight normalisation (modules/conv.py:47-88: the norm is recomputed every
 * step; scripts/train.py:1421-1480).  ALL pointers are DEVICE pointers (parameters live on the GPU while training); gradients have the
 * shapes of what they differentiate.  The weight-norm fold runs on the device in every call (forward and backward both fold). */

/* The general fused unit of the encoder/decoder trunk, forward and backward:
 *     y[B,M,Tout] = DW_{ks,stride}( (g_pw v_pw/||v_pw||) @ act(pre_scale * x[B,K,Tin]) ; g_dw v_dw/||v_dw|| ) + bias
 * act = ELU (pre_elu = 1) or identity; causal SConv1d geometry (conv.py:715-763): left pad ks - stride, Tout = ceil(Tin/stride).
 * K = M = C, ks = 5, stride = 1, pre_elu = 1 is one half of a SEANetResnetBlock (modules/seanet.py:39-116 dws_conv_block); M = 2K,
 * ks = 2r, stride = r is the encoder's Downsample unit (seanet.py:733-772).  v_pw [M,K], v_dw [M,ks]; ks <= 16.  dx may be NULL (first
 * layer: no input gradient).  Any K, M and Tin: shapes off the LDS-DMA core's grid (C <= 32, T % 4 != 0) run on the round-1 core. */
typedef struct wv_train_unit wv_train_unit;
int wv_train_unit_create(int K, int M, int ks, int stride, wv_train_unit** out);
void wv_train_unit_destroy(wv_train_unit* u);
size_t wv_train_unit_workspace_bytes(const wv_train_unit* u, int B, int Tin);   /* backward only */
int wv_train_unit_forward(wv_train_unit* u, const float* x, const float* g_pw, const float* v_pw, const float* g_dw,
                          const float* v_dw, const float* bias, float pre_scale, int pre_elu, float* y, int B, int Tin, void* stream);
int wv_train_unit_backward(wv_train_unit* u, const float* x, const float* g_pw, const float* v_pw, const float* g_dw,
                           const float* v_dw, float pre_scale, int pre_elu, const float* dy, float* dx, float* dg_pw, float* dv_pw,
                           float* dg_dw, float* dv_dw, float* db, int B, int Tin, void* workspace, size_t workspace_bytes, void* stream);

/* Whole SEANetResnetBlock with live weight norm (modules/seanet.py:245-281, identity shortcut):
 *     y = x + s * half2(half1(pre_scale * x)),   s = res_scale * res_scale_param[0]  (res_scale_param may be NULL: s = res_scale)
 * forward keeps the two intermediate activations and the two 1x1 outputs in `saved` (wv_train_block_saved_bytes: four activation-sized
 * tensors; the forward kernels store the 1x1 outputs themselves, backward then has no GEMM to recompute) for backward, which returns
 * dx, both halves' parameter gradients and d(res_scale_param).  Both halves are units with K = M = C, ks = 5, stride = 1.
 * CONTRACT: wv_train_block_backward reuses the weight folds (W, its packed copies, 1/||v||) that the forward left in the handle, so it
 * must follow the wv_train_block_forward that produced `saved` with the SAME parameter tensors, and nothing may change their values or
 * run another forward on this handle in between (optimizer steps come after backward).  Other parameter pointers fail with WV_ESTATE. */
typedef struct wv_train_block wv_train_block;
typedef struct { const float *g_pw, *v_pw, *g_dw, *v_dw, *bias; } wv_half_params;     /* device pointers */
typedef struct { float *dg_pw, *dv_pw, *dg_dw, *dv_dw, *db; } wv_half_grads;          /* device pointers */
int wv_train_block_create(int C, wv_train_block** out);
void wv_train_block_destroy(wv_train_block* b);
size_t wv_train_block_saved_bytes(const wv_train_block* b, int B, int T);
size_t wv_train_block_workspace_bytes(const wv_train_block* b, int B, int T);       /* backward only */
int wv_train_block_forward(wv_train_block* b, const float* x, const wv_half_params* p /*[2]*/, const float* res_scale_param,
                           float pre_scale, float res_scale, float* y, void* saved, size_t saved_bytes, int B, int T, void* stream);
int wv_train_block_backward(wv_train_block* b, const float* x, const wv_half_params* p /*[2]*/, const float* res_scale_param,
                            float pre_scale, float res_scale, const float* dy, const void* saved, float* dx,
                            const wv_half_grads* g /*[2]*/, float* d_res_scale_param, int B, int T,
                            void* workspace, size_t workspace_bytes, void* stream);

/* conv_pre with live weight norm (seanet.py:657-664): y[B,C,T] = causal conv1d(in_scale * x[B,1,T], g v/||v|| [C,1,ks]) + bias.
 * backward: dg [C], dv [C,ks], db [C] and, optionally, dx [B,1,T] (the gradient towards the audio; NULL to skip). */
typedef struct wv_train_convpre wv_train_convpre;
int wv_train_convpre_create(int C, int ks, wv_train_convpre** out);
void wv_train_convpre_destroy(wv_train_convpre* h);
size_t wv_train_convpre_workspace_bytes(const wv_train_convpre* h, int B, int T);
int wv_train_convpre_forward(wv_train_convpre* h, const float* x, const float* g, const float* v, const float* bias, float in_scale,
                             float* y, int B, int T, void* stream);
int wv_train_convpre_backward(wv_train_convpre* h, const float* x, const float* g, const float* v, float in_scale, const float* dy,
                              float* dx, float* dg, float* dv, float* db, int B, int T, void* workspace, size_t workspace_bytes, void* stream);

/* SpecBlock add with live weight norm (seanet.py:463-511): y[B,C,T] = x + s * ((g v/||v||)[C,F] @ P[B,F,T]),
 * s = res_scale * scale_param[0] (scale_param: device scalar of zero_init blocks, or NULL).  P is the normalised
 * log-magnitude STFT of the waveform (no parameters; wv_op_stft_logmag / the model's STFT kernel).  dx = dy (identity)
 * is the caller's; backward returns dg [C], dv [C,F], d(scale_param) and, when asked, dP = s W^T dy (the gradient towards the
 * features, continued to the audio by wv_stft_plan_backward).  y may alias x. */
typedef struct wv_train_spec wv_train_spec;
int wv_train_spec_create(int C, int F, wv_train_spec** out);
void wv_train_spec_destroy(wv_train_spec* h);
size_t wv_train_spec_workspace_bytes(const wv_train_spec* h, int B, int T);
int wv_train_spec_forward(wv_train_spec* h, const float* x, const float* P, const float* g, const float* v, const float* scale_param,
                          float res_scale, float* y, int B, int T, void* stream);
int wv_train_spec_backward(wv_train_spec* h, const float* P, const float* g, const float* v, const float* scale_param, float res_scale,
                           const float* dy, float* dg, float* dv, float* d_scale_param, float* dP /* [B,F,T] or NULL */, int B, int T,
                           void* workspace, size_t workspace_bytes, void* stream);

/* conv_post with live weight norm (seanet.py:795-822): y[B,D,T] = L2Norm( (g_pw v_pw/||v_pw||)[D,C] @ DW_ks( ELU(x[B,C,T]) ; g_dw v_dw/||v_dw|| ) + bias )
 * L2Norm = x / max(||x||_2 over channels, 1e-12) * sqrt(D) (seanet.py:288-318; l2norm = 0 skips it).  D <= 128.
 * v_dw [C,ks] (no bias on the depth-wise conv), v_pw [D,C], bias [D]. */
typedef struct wv_train_convpost wv_train_convpost;
int wv_train_convpost_create(int C, int D, int ks, wv_train_convpost** out);
void wv_train_convpost_destroy(wv_train_convpost* h);
size_t wv_train_convpost_workspace_bytes(const wv_train_convpost* h, int B, int T);
int wv_train_convpost_forward(wv_train_convpost* h, const float* x, const float* g_dw, const float* v_dw, const float* g_pw, const float* v_pw,
                              const float* bias, int l2norm, float* y, int B, int T, void* stream);
int wv_train_convpost_backward(wv_train_convpost* h, const float* x, const float* g_dw, const float* v_dw, const float* g_pw, const float* v_pw,
                               const float* bias, int l2norm, const float* dy, float* dx, float* dg_dw, float* dv_dw, float* dg_pw, float* dv_pw,
                               float* db, int B, int T, void* workspace, size_t workspace_bytes, void* stream);

/* Detector / locator head (model/detector.py:209-218,278-318; locator.py likewise): plain (not weight-normed) parameters
 *   logits[B,nb,T] = Conv1d(O, nb, 1)( ConvTranspose1d(D, O, k = s = hop)(z[B,D,N])[:, :, :T] ),  T <= N * hop
 * w_rev [D,O,hop], b_rev [O], w_last [nb,O], b_last [nb].  (Inference composes the two layers into one weight; training keeps
 * them apart so that each gets its gradient.) */
typedef struct wv_train_head wv_train_head;
int wv_train_head_create(int D, int O, int nb, int hop, wv_train_head** out);
void wv_train_head_destroy(wv_train_head* h);
size_t wv_train_head_workspace_bytes(const wv_train_head* h, int B, int N);
int wv_train_head_forward(wv_train_head* h, const float* z, const float* w_rev, const float* b_rev, const float* w_last, const float* b_last,
                          float* logits, int B, int N, int T, void* workspace, size_t workspace_bytes, void* stream);
int wv_train_head_backward(wv_train_head* h, const float* z, const float* w_rev, const float* b_rev, const float* w_last, const float* dlogits,
                           float* dz, float* dw_rev, float* db_rev, float* dw_last, float* db_last, int B, int N, int T,
                           void* workspace, size_t workspace_bytes, void* stream);

/* The decoder's upsample unit with live weight norm (seanet.py:1110-1135; conv.py:838-881):
 *   y[B,M,r*Tin] = (g_pw v_pw/||v_pw||)[M,K] @ ConvTranspose1d_depthwise(act(pre_scale * x[B,K,Tin]); g_ct v_ct/||v_ct|| [K,2r], stride r) + bias
 * (causal: the last r samples of the transposed conv are trimmed).  ratio <= 8. */
typedef struct wv_train_up wv_train_up;
int wv_train_up_create(int K, int M, int ratio, wv_train_up** out);
void wv_train_up_destroy(wv_train_up* h);
size_t wv_train_up_workspace_bytes(const wv_train_up* h, int B, int Tin);
int wv_train_up_forward(wv_train_up* h, const float* x, const float* g_ct, const float* v_ct, const float* g_pw, const float* v_pw, const float* bias,
                        float pre_scale, int pre_elu, float* y, int B, int Tin, void* stream);
int wv_train_up_backward(wv_train_up* h, const float* x, const float* g_ct, const float* v_ct, const float* g_pw, const float* v_pw, float pre_scale,
                         int pre_elu, const float* dy, float* dx, float* dg_ct, float* dv_ct, float* dg_pw, float* dv_pw, float* db, int B, int Tin,
                         void* workspace, size_t workspace_bytes, void* stream);

/* The decoder's tail with live weight norm (seanet.py:1166-1204; generator.py:396-413 trims to T):
 *   delta[B,1,T] = tanh( wav_std * ( causal conv1d(ELU(post * x[B,C,Tin]), g v/||v|| [1,C,ks]) + bias ) )[..., :T],  T <= Tin
 * (the watermarked audio is delta + the input clip: watermarking.py:423-441).  g [1], v [1,C,ks] (norm over the whole tensor). */
typedef struct wv_train_tail wv_train_tail;
int wv_train_tail_create(int C, int ks, wv_train_tail** out);
void wv_train_tail_destroy(wv_train_tail* h);
size_t wv_train_tail_workspace_bytes(const wv_train_tail* h, int B);
int wv_train_tail_forward(wv_train_tail* h, const float* x, const float* g, const float* v, const float* bias, float post, float wav_std,
                          float* delta, int B, int Tin, int T, void* stream);
int wv_train_tail_backward(wv_train_tail* h, const float* x, const float* g, const float* v, float post, float wav_std, const float* delta,
                           const float* d_delta, float* dx, float* dg, float* dv, float* db, int B, int Tin, int T,
                           void* workspace, size_t workspace_bytes, void* stream);

/* Message MLP + FiLM (seanet.py:518-550,831-846,905-966).  `params` / `dparams` are one packed block:
 *   W0 [E][msg_dim], b0 [E], layers x (W [E][E], b [E]), FW [n_scales][bands][2][E] (gamma row, beta row), FB [n_scales][bands][2]
 * (wv_train_film_param_count floats).  film[B][n_scales][bands][2] = (gamma, beta) per clip, scale and frequency band;
 *   e0 = W0 msg + b0, e_l = relu(W_l e_{l-1} + b_l), gamma/beta = <FW, e_L> + FB.
 * wv_train_film_apply: y[b,c,t] = x * gamma[b][scale][band(c)] + beta (band = c / (C / bands));  its backward returns dx and fills
 * dfilm's entries of `scale`; wv_train_film_backward turns the complete dfilm into parameter gradients (ws = forward's buffer). */
size_t wv_train_film_param_count(int msg_dim, int E, int layers, int n_scales, int bands);
size_t wv_train_film_workspace_bytes(int B, int msg_dim, int E, int layers, int n_scales, int bands);
int wv_train_film_forward(const float* msg, const float* params, float* film, int B, int msg_dim, int E, int layers, int n_scales, int bands,
                          void* workspace, size_t workspace_bytes, void* stream);
int wv_train_film_backward(const float* msg, const float* params, const float* dfilm, float* dparams, int B, int msg_dim, int E, int layers,
                           int n_scales, int bands, void* workspace, size_t workspace_bytes, void* stream);
int wv_train_film_apply(const float* x, const float* film, float* y, int B, int C, int T, int bands, int n_scales, int scale, void* stream);
int wv_train_film_apply_backward(const float* x, const float* film, const float* dy, float* dx, float* dfilm, int B, int C, int T, int bands,
                                 int n_scales, int scale, void* workspace, size_t workspace_bytes, void* stream);

/* The two BCE-with-logits losses of the training step (scripts/loss.py:947-1099), forward + gradient in one pass:
 *   LocalizationLoss: msg = NULL, Cz = 1:  mean BCE(logits[B,1,T], mask[B,1,T])
 *   DecodingLoss:     mean BCE(logits[B,Cz,T], msg[B,Cz] * mask[B,1,T])        (mask NULL = all ones)
 * loss: one device float; dlogits (optional, [B,Cz,T]) = grad_scale * dLoss/dlogits.  Fixed-order two-stage sum. */
size_t wv_train_bce_workspace_bytes(void);
int wv_train_bce_logits(const float* logits, const float* mask, const float* msg, float* loss, float* dlogits, float grad_scale,
                        int B, int Cz, int T, void* workspace, size_t workspace_bytes, void* stream);
/* Waveform loss of the generator update (scripts/train.py:1322, audiotools L1Loss): loss = mean |a - b|, da (optional) =
 * grad_scale * sign(a - b) / n.  Workspace: wv_train_bce_workspace_bytes(). */
int wv_train_l1(const float* a, const float* b, float* loss, float* da, float grad_scale, size_t n, void* workspace, size_t workspace_bytes, void* stream);

/* The training units' live weight-norm fold on its own: w[m][k] = g[m] * v[m][k] / ||v[m]||, inv_norm[m] = 1 / ||v[m]|| (modules/conv.py:73-74:
 * the norm runs over all dimensions but the first; K = their product).  The same device code folds the weights inside every training
 * forward, so a trained net written out in the reference's STRIPPED checkpoint layout (scripts/train.py:1624-1629 removes the
 * parametrizations before saving) holds exactly the weights the training forward used.  g [M], v [M][K], w [M][K], inv_norm [M]: device pointers. */
int wv_train_fold_weight(const float* g, const float* v, float* w, float* inv_norm, int M, int K, void* stream);

/* Optimizer step over FLAT device arenas (a net's parameters / gradients / AdamW moments are contiguous; scripts/train.py:1346-1358,
 * conf/base.yml:128-130): wv_train_sumsq = sum of squares of the gradient arena (fixed-order two-stage sum; device scalar `out`);
 * wv_train_adamw = torch.nn.utils.clip_grad_norm_(max_norm) -- when grad_sumsq is given -- followed by torch.optim.AdamW's
 * update at 1-based step `step`; the ExponentialLR schedule is the caller's lr. */
int wv_train_sumsq(const float* g, size_t n, float* out, void* workspace, size_t workspace_bytes /* wv_train_bce_workspace_bytes() */, void* stream);
int wv_train_adamw(float* p, const float* g, float* m, float* v, size_t n, float lr, float beta1, float beta2, float eps,
                   float weight_decay, int step, const float* grad_sumsq, float max_norm, void* stream);

/* ==== csrc/wv_metrics.hip: per-clip metrics of a validation pass (semantics in waveverify_amd/metrics.py) ---------------------
 * Three single-pass reductions, each with a caller-provided workspace sized by its *_workspace_bytes query (0 = bad shape).  Device
 * pointers, contiguous; inputs may sit on any 4-byte boundary, the workspace and the double outputs on 8.  Rows are summed in chunks
 * of 4096 samples in a fixed order, in f64 (or int32), and the chunks in ascending order: results are bit-identical from run to run
 * and a clip's result does not depend on the batch it is part of.  B * W and B <= 65535.
 *
 * decode = scripts/evaluate.py BER.forward :442-516 up to the per-clip counts.  logits [B,W,T], bits [B,W] (float 0 / 1), mask [B,1,T]
 * or NULL.  Per (clip, bit) S = sum sigmoid(l) * m and N = sum m are rounded to f32 and finished in f32 as the reference writes it:
 * avg = S / (N + eps), valid = N > 0; without a mask avg = S / T and every bit is valid.  decoded = avg >= threshold.
 * Outputs: avg [B,W] float, errors [B] int32 (valid bits with decoded != bit), valid [B] int32 (valid bits). */
size_t wv_metrics_decode_workspace_bytes(int B, int W, int T);
int wv_metrics_decode(const float* logits, const float* bits, const float* mask, float threshold, float eps, int B, int W, int T, float* avg,
                      int* errors, int* valid, void* workspace, size_t workspace_bytes, void* stream);
/* iou = the counts of MIOU.forward :591-665 on p = (pred > 0.5) (the RAW locator output, model/watermarking.py:797) and the 0 / 1 mask g:
 * counts [B][4] int32 = |p and g=1|, |p or g=1|, |not p and g=0|, |not p or g=0|.  pred, mask [B,1,T]. */
size_t wv_metrics_iou_workspace_bytes(int B, int T);
int wv_metrics_iou(const float* pred, const float* mask, int B, int T, int* counts, void* workspace, size_t workspace_bytes, void* stream);
/* sisnr = SISNR.forward :167-229 per clip.  estimate, reference [B,1,T].  moments [B][5] double = sum x, sum y, sum xx, sum xy, sum yy
 * (x = estimate, y = reference); sisnr [B] double = 10 log10(|proj|^2 / (|x0 - proj|^2 + eps) + eps) in dB with x0, y0 the zero-meaned
 * signals and proj = y0 [x0.y0] / (|y0|^2 + eps), evaluated on the moments in f64. */
size_t wv_metrics_sisnr_workspace_bytes(int B, int T);
int wv_metrics_sisnr(const float* estimate, const float* reference, int B, int T, double eps, double* sisnr, double* moments, void* workspace,
                     size_t workspace_bytes, void* stream);

/* ==== csrc/wv_stoi.hip: STOI per clip (Taal et al. 2011, non-extended; the algorithm and its constants in waveverify_amd/stoi.py) ----
 * reference (the CLEAN clip: the silent frames are its, and the measure is not symmetric) and estimate [B,1,T], device pointers on any
 * 4-byte boundary.  Both go to 10 kHz through wv_fx_resample with `kernels` [up][L] (orig = down, nw = up, L, width as documented there;
 * stoi.resample_kernels builds the table of Octave's `resample` filter); kernels = NULL with up == down means the clips are at 10 kHz.
 * basis: [256][512] float followed by 256 window samples (stoi.dft_basis: bins 7..218 of the 512-point DFT, re / im interleaved, the Hann
 * window folded in, zero rows behind), built on the host in float64 and kept by the caller.  Outputs, every element written:
 *   stoi     [B] double, 8-byte aligned: d, or 1e-5 where fewer than 30 frames are left
 *   frames   [B][2] int32: frames kept, frames of the 10 kHz clip (F = ceil((ceil(T up / down) - 256) / 128), 0 under 257 samples)
 *   kept_idx optional [B][F] int32: the kept frames' indices ascending, then -1
 *   tob      optional [B][2][15][F - 1] float: third-octave magnitudes of reference and estimate, zeros behind a clip's kept - 1 frames
 * NULL = not written.  Sums run in fixed orders without atomics (frame energies, band sums and the correlation in f64; the DFT as an
 * f32 fmaf chain on the matrix pipe): two runs are bit-equal and a clip's numbers do not depend on its batch.  B <= 65535. */
size_t wv_metrics_stoi_workspace_bytes(int B, int T, int up, int down, int L, int width);
int wv_metrics_stoi(const float* reference, const float* estimate, int B, int T, const float* kernels, int up, int down, int L, int width,
                    const float* basis, double* stoi, int* frames, int* kept_idx, float* tob, void* workspace, size_t workspace_bytes,
                    void* stream);

/* ==== csrc/wv_loudness.hip: ITU-R BS.1770-4 gated loudness of windows of one arena, and the loudness-gated batch draw ---------
 * Not the reference's own arithmetic (it measures through audiotools / pyloudnorm, scripts/train.py:440-475): a restatement of the
 * published standard; the constants and the float64 statement are in waveverify_amd/loudness.py.  One channel.
 *
 * wv_loudness measures N windows of T samples that live anywhere in the f32 arena `pool` (they may overlap; a plain batch [B,1,T] is
 * starts[b] = b T).  Device pointers:
 *   starts  [N] int64: sample offset of a window in pool
 *   lens    [N] int32: its valid samples, clamped to [0, T]; the rest of the window counts as zeros, and nothing at or past
 *           pool + starts + lens is read
 *   table   12 doubles from loudness.device_table(fs): the K-weighting as 2 x 6 [b0 b1 b2 1 a1 a2] (shelf, then high-pass; scipy's sos
 *           layout), computed on the host in float64
 * fs % 10 == 0, 4 (fs / 10) <= T <= 2^30.  The filter state is zero at every window's first sample.  Outputs:
 *   lufs     [N] double: -0.691 + 10 log10(mean z of the blocks past both gates), -70.0 where no block passes the absolute gate
 *   sub      [N][T / (fs / 10)] double: sum of squares of the K-weighted signal over each whole 100 ms sub-block; block j is
 *            sub-blocks j..j+3, z_j their sum / (4 fs / 10)
 *   filtered optional [N][T] float: the K-weighted signal (f64 rounded once); NULL = not written
 * starts, table, lufs and sub on 8-byte boundaries.  A lane per window runs the recurrence sample by sample in f64 in scipy.signal.sosfilt's
 * order of operations (the nearly double high-pass pole makes every other order differ from it by 1e-11 .. 4e-10 where only the filter
 * rings); the lanes of a wave share coalesced loads through LDS in chunks of wv_loudness_chunk() samples.  Sums in sample and block order,
 * no atomics: runs are bit-equal and a window's numbers depend neither on N nor on its row.  The kernel keeps its intermediates in LDS;
 * the workspace is reserved (its query gives 0 for a refused shape), and one shorter than the query is a bad argument like the others:
 * WV_EINVAL, nothing written.
 *
 * wv_pool_sample: starts, lens [B][tries], lufs [B][tries] double or NULL.  choice[b] = the first try k with lufs[b][k] > cutoff, else
 * tries - 1 (lufs == NULL: 0); out [B,1,T] float = window (b, choice[b]) copied, zeros past its length.  One launch; B <= 65535. */
int wv_loudness_chunk(void);
size_t wv_loudness_workspace_bytes(int N, int T, int fs);
int wv_loudness(const float* pool, const int64_t* starts, const int32_t* lens, int N, int T, int fs, const double* table, double* lufs,
                double* sub, float* filtered, void* workspace, size_t workspace_bytes, void* stream);
int wv_pool_sample(const float* pool, const int64_t* starts, const int32_t* lens, const double* lufs, int B, int tries, int T, double cutoff,
                   float* out, int32_t* choice, void* stream);

/* ==== csrc/wv_aug.hip: temporal augmentations of the training step ------------------------------------
 * One bandwidth-bound pass that replaces the reference's per-clip / per-segment Python loops and its GPU->CPU->GPU
 * hop (model/watermarking.py:487-519,540).  All pointers are DEVICE pointers, tensors [B,C,T] contiguous f32.
 *
 * wv_aug_localize_sequence = LocalizationAugmentation.forward (utils/localization_augmentation.py:212-321) followed
 * by SequenceAugmentation.forward (utils/seq_augmentation.py:100-273), i.e. AudioWatermarking._apply_augmentations:
 *   plan  int32 [B][nseg], nseg = ceil(T / seg_len): what happens to segment s of clip b --
 *         0 keep | 1 revert to the original | 2 replace by zeros | 3 + j substitute clip j's ORIGINAL (0 <= j < B);
 *         NULL = no localisation augmentation.  The host draws it (waveverify_amd/augment.py, same RNG call order
 *         as the reference) and validates j.
 *   seq_* the sequence map applied afterwards (WV_SEQ_*); out[t] = in[src(t)] for all three outputs:
 *         REVERSE: torch.flip;  ROLL: torch.roll(shifts = seq_a), 0 < seq_a < T;
 *         PERMUTE: segments of seq_a samples, output segment i = input segment perm[i] (device int32, T_out / seq_a
 *                  entries, the caller validates the range); T_out = n_segments * seq_a <= T (the reference drops the tail);
 *         CHUNK_SWAP: chunks [seq_a, seq_a + seq_c) and [seq_b, seq_b + seq_c) exchanged (non-overlapping).
 *   outputs: wm_out (augmented watermarked), orig_out (updated original), mask_out (1 = watermark present), [B,C,T_out].
 * wv_aug_sequence applies only the sequence map to up to three [rows,T] tensors (NULL inputs are skipped). */
#define WV_SEQ_IDENTITY 0
#define WV_SEQ_REVERSE 1
#define WV_SEQ_ROLL 2
#define WV_SEQ_PERMUTE 3
#define WV_SEQ_CHUNK_SWAP 4
int wv_aug_localize_sequence(const float* original, const float* watermarked, const int* plan, int nseg, int seg_len,
                             int seq_mode, int seq_a, int seq_b, int seq_c, const int* perm,
                             float* wm_out, float* orig_out, float* mask_out, int B, int C, int T, int T_out, void* stream);
/* gradient of the augmented audio towards the watermarked input: d_wm[b,c,ts] = d_out[b,c,t] where out[t] was copied from wm[ts]
 * (plan code 0), else 0.  inv_* = the INVERSE of the forward's sequence map (reverse and chunk swap are their own inverses; roll by a
 * -> roll by T - a; permutation -> its inverse permutation). */
int wv_aug_backward(const float* d_out, const int* plan, int nseg, int seg_len, int inv_mode, int inv_a, int inv_b, int inv_c, const int* inv_perm,
                    float* d_wm, int B, int C, int T, int T_out, void* stream);
int wv_aug_sequence(const float* in0, const float* in1, const float* in2, float* out0, float* out1, float* out2,
                    int seq_mode, int seq_a, int seq_b, int seq_c, const int* perm, int rows, int T, int T_out, void* stream);

/* ==== csrc/wv_fx.hip: sinc-filter / resample effects -------------------------------------------------------------
 * A FIR filter bank over a padded signal (device pointers):  y[row][f][n] = sum_j taps[f][j] * xpad[n*stride + j], n < Tout =
 * (T + pad_l + pad_r - L) / stride + 1; replicate = 1 pads with the edge samples (julius' filters), 0 with zeros (the polyphase resampler);
 * interleave = 1 stores y[row][n*n_filters + f].  n_filters <= 8.  The taps are built on the host the way julius 0.2.7 / torchaudio
 * publish them (waveverify_amd/effects.py) -- third-party arithmetic that is not in this image: parity with the libraries is UNPINNED. */
int wv_fx_fir_bank(const float* x, const float* taps, float* y, int rows, int T, int n_filters, int L, int stride, int pad_l, int pad_r,
                   int replicate, int interleave, void* stream);
/* Adjoints of the two effects (the reference's julius filters and torchaudio resampler are plain differentiable torch ops --
 * utils/effect_augmentation.py:1451-1501,1684-1870 -- so a loss gradient crosses them through the TRANSPOSED operator):
 * the transpose of wv_fx_fir_bank with stride 1 is the same call on dy with time-reversed taps and L-1 zeros of padding on both sides
 * (giving the gradient towards the PADDED signal), followed by wv_fx_fold_replicate, the transpose of the replicate padding:
 * dx[t] = dxp[t + pad_l], with the pad samples' gradients added to dx[0] / dx[T-1].  dxp [rows][T + pad_l + pad_r], dx [rows][T]. */
int wv_fx_fold_replicate(const float* dxp, float* dx, int rows, int T, int pad_l, int pad_r, void* stream);
/* transpose of wv_fx_resample: dx[row][s] = sum_{m = n*new + f < Tout, j : n*orig + j - width = s} kernels[f][j] * dy[row][m];  dy [rows][Tout], dx [rows][T] */
int wv_fx_resample_adjoint(const float* dy, const float* kernels, float* dx, int rows, int T, int orig, int new_, int L, int width, int Tout,
                           void* stream);
/* polyphase sinc resampling by orig : nw (both already divided by their gcd), torchaudio's formulation: kernels [nw][L], L = 2*width + orig;
 * y[row][m] = sum_j kernels[m % nw][j] * xz[(m / nw)*orig + j - width] for m < Tout = ceil(nw * T / orig), xz zero outside [0,T).
 * Any 1 <= Tout <= (ceil(T / orig) + 1) * nw is served (the same formula, continued or cut short); a longer one is refused. */
int wv_fx_resample(const float* x, const float* kernels, float* y, int rows, int T, int orig, int nw, int L, int width, int Tout, void* stream);

/* ==== csrc/wv_native.hip: the two ends of the native-rate embed route ---------------------------------------------
 * A file of C channels at its own rate goes to the model's 16 kHz mono, and the model's 16 kHz residual comes back onto every channel,
 * one kernel each.  The resampler is wv_fx_resample's (orig : nw divided by their gcd, L = 2*width + orig, output m = n*nw + f reads inputs
 * n*orig - width + j, j < L, zero outside the signal; one fmaf chain per output in ascending j from +0), but the table arrives TRANSPOSED:
 * kernels_t [L][nw], kernels_t[j][f] = kernels[f][j].  orig = nw = L = 1, width = 0, kernels_t = {1} is the identity resampler.
 * Planar device tensors on any 4-byte boundary.  Refused with nothing launched and nothing written: a null pointer, B outside [1, 65535],
 * C outside [1, 64], a length, orig, nw or L below 1, width < 0, an output longer than (ceil(T_in / orig) + 1) * nw (T_in = Tn for the front
 * end, T16 for the back end), or a ratio whose 256-output tile reads more than 64 KB of input: ((nw + 254) / nw) * orig + L > 16384 floats.
 *   front end: x [B][C][Tn] -> y [B][Tout];  mono[s] = (x[b][0][s] + x[b][1][s] + ...) / (float)C, summed left to right in f32 and divided
 *              exactly, formed on the way into the kernel's LDS window (no mono tensor is written);  y[b][m] = the chain over mono.
 *   back end:  delta [B][T16], x and out [B][C][Tn];  u[b][m] = the chain over delta, once per m < Tn;  out[b][c][m] = x[b][c][m] +
 *              gain * u[b][m] with both roundings kept (gain = 1 gives x + u).  out may be x: each element is read, then written, by the
 *              same thread. */
int wv_native_downmix_resample(const float* x, const float* kernels_t, float* y, int B, int C, int Tn, int orig, int nw, int L, int width, int Tout,
                               void* stream);
int wv_native_upsample_add(const float* x, const float* delta, const float* kernels_t, float* out, int B, int C, int T16, int Tn, int orig, int nw, int L,
                           int width, float gain, void* stream);

/* ---- csrc/wv_channel_floor.hip: the back end under a PER-CHANNEL SNR floor at the file's own rate (DESIGN.md section 7d-12;
 * waveverify_amd/channel_floor.py is the definition, bit for bit).  x, delta, kernels_t, out, B .. width: wv_native_upsample_add's, and u[b][m] is
 * that call's fmaf chain through the same device function.  hop: the generator's hop at 16 kHz; rho = 10^(-min_snr_db / 10); strengths [B] f32
 * DEVICE, the cap s of each row; add 0 / 1; gains: null, or [B][C][F] f32 DEVICE that takes every g; F = ((Tn - 1) * orig) / (nw * hop) + 1.
 *   native sample m belongs to frame (m * orig) / (nw * hop) in int64: frame f is [start(f), start(f + 1)) cut at Tn, start(f) = ceil(f * nw *
 *     hop / orig), its nominal length L_f = start(f + 1) - start(f) (lengths differ by at most one; a frame may be empty where nw * hop < orig);
 *   Ex[c][f] = sum x[b][c]^2, Eu[f] = sum u[b]^2 over the frame in float64, in wv_snr_floor's fixed order with k counted inside the frame;
 *   g[c][f] = s where Eu == 0, else q < (double)s ? (float)q : s with q = sqrt((rho * Ex) / Eu), divide and square root correctly rounded;
 *   w = g_prev < g[c][f] ? min(g[c][f], g_prev + (g[c][f] - g_prev) * ramp) : g[c][f] in f32, every rounding kept, g_prev = g[c][f - 1] (frame 0:
 *     g[c][0]), ramp = float32((k + 1) / L_f) formed in float64 and rounded once;
 *   v = w * u;  add == 0: out = v;  add == 1: out = x + v, but x's own bits where v is +0 or -0.
 * Two launches: the first reads x and delta and fills the workspace (u [B][Tn], then g [B][C][F], each on a 256-byte boundary), the second reads
 * the workspace and x and writes out.  out may be x: each element is read for its last time, then written, by the same thread of the second
 * launch.  The workspace is the caller's, on a 256-byte boundary, at least wv_native_floor_up_add_bytes(...) bytes, contents undefined before
 * and after.  A row whose strength is negative, infinite or not a number is SKIPPED whole; the other rows are served.
 * Refused with WV_EINVAL, nothing launched and nothing written: everything wv_native_upsample_add refuses; null strengths or workspace; hop < 1;
 * nw * hop or F beyond 2^31 - 1; rho not finite or <= 0; add not 0 or 1; a workspace that is misaligned or too small; a frame of
 * ceil(nw * hop / orig) > WV_CHANNEL_FLOOR_MAX_FRAME native samples, or one that together with the 256-output input window
 * (((nw + 254) / nw) * orig + L floats) passes WV_CHANNEL_FLOOR_LDS_FLOATS: the first launch holds both in LDS. */
#define WV_CHANNEL_FLOOR_MAX_FRAME 4096
#define WV_CHANNEL_FLOOR_LDS_FLOATS 15360
int wv_native_floor_up_add_bytes(int B, int C, int T16, int Tn, int orig, int nw, int L, int width, int hop, size_t* workspace_bytes);
int wv_native_floor_up_add(const float* x, const float* delta, const float* kernels_t, float* out, int B, int C, int T16, int Tn, int orig, int nw, int L,
                           int width, int hop, double rho, const float* strengths, int add, float* gains, void* workspace, size_t workspace_bytes,
                           void* stream);

/* ---- the same two ends for live sessions: S streams in lockstep, one launch per end and push, the state on the device.
 * A stage's sequence is cat(history[s][0 .. hv), new[s][0 .. n)), never materialised.  Output 0 of a call is phase 0 of the first phase group the
 * stream has not emitted yet, and its first tap is sequence sample -pad (0 <= pad <= width; pad > 0 only while the stream's start lies inside the
 * filter): output m = g * nw + f is the file kernels' fmaf chain over sequence samples g * orig - pad + j, j < L, zero outside the sequence.  The
 * caller (waveverify_amd/native_session.py) asks only for outputs all of whose taps have arrived, or, at flush, for the rest with zeros past the end.
 * Next-state buffers are second buffers, never their sources; a next state is the sequence's last samples: drop + hv2 == hv + n.  Any of n, n_out,
 * nr, k, hv2, rv2 may be 0 (its pointer may then be null); with nothing to write nothing is launched.
 *   front:  hist, hist_out [S][hcap] hold channel MEANS; x [S][C][n] new planar samples, whose mean is formed as wv_native_downmix_resample forms
 *           it; y [S][n_out]; hist_out[s][0 .. hv2) = sequence samples [drop, drop + hv2).
 *   back:   rhist, rhist_out [S][rcap] and r [S][nr] the 16 kHz residual (rhist_out = its samples [rdrop, rdrop + rv2), rdrop + rv2 == rv + nr);
 *           pend, pend_out [S][C][pcap] the delay line of original samples not yet emitted and x [S][C][n] the new ones;
 *           out[s][c][i] = cat(pend[s][c][0 .. pv), x[s][c])[i] + gain * u[s][i] for i < k <= pv + n, both roundings kept; pend_out[s][c] = that
 *           sequence's samples [k, pv + n), at most pcap of them.
 * Refused with WV_EINVAL, nothing launched or written: a null pointer that is needed, a next-state buffer equal to its source, S outside [1, 65535],
 * C outside [1, 64], orig, nw or L < 1, width < 0, pad outside [0, width], a valid or next length outside [0, capacity], a negative count, more
 * outputs than (ceil((pad + sequence) / orig) + 1) * nw, k > pv + n, or a 256-output tile whose input window passes 64 KB of LDS. */
int wv_native_session_down(const float* hist, int hcap, int hv, const float* x, int n, const float* kernels_t, float* y, int n_out, int pad,
                           float* hist_out, int drop, int hv2, int S, int C, int orig, int nw, int L, int width, void* stream);
int wv_native_session_up_add(const float* rhist, int rcap, int rv, const float* r, int nr, const float* kernels_t, const float* pend, int pcap, int pv,
                             const float* x, int n, float* out, int k, int pad, float gain, float* pend_out, float* rhist_out, int rdrop, int rv2,
                             int S, int C, int orig, int nw, int L, int width, void* stream);

/* ---- and for session BANKS (waveverify_amd/native_bank.py): up to `capacity` slots, each a stream with its OWN rate, channel
 * count, packet length and resampler state; the P slots a tick names are served by one launch per stage, whatever the mix of rates.
 * A RATE TABLE is a host array of at most WV_NATIVE_BANK_MAX_RATES entries, one resampler each (kernels_t a DEVICE pointer to the transposed table
 * [L][nw] described above).  The entry point copies the table into the kernel's arguments by value; a descriptor names a rate by its index.  The
 * launch's LDS is the largest 256-output window of the table, and an entry whose window passes 64 KB is refused as above.
 * STATE is ping-pong per slot, so that no launch reads and writes the same bytes:  hist [capacity][2][hcap] (channel means),
 * rhist [capacity][2][rcap], pend [capacity][2][Cmax][pcap].  A descriptor's `half` names the half that holds the slot's current state; the launch
 * reads it and writes the next state into the other half, and the caller flips its bit for every slot a call named.  Slots that no descriptor names
 * are not touched, and the work grows with the rows and samples pushed, not with capacity.  The slots of one call must be distinct (the caller's
 * duty, as for wv_bank_advance: two rows of one slot would race on its next state).
 * Descriptors are int64 rows on the device; offsets count floats in the call's arenas, which hold planar [C][count] blocks:
 *   wv_native_bank_down    desc [P][12] = {slot, rate, C, hv, x_off, n, y_off, n_out, pad, drop, hv2, half}: the row's new samples are C planar
 *                          channels of n floats at x + x_off, its n_out outputs go to y + y_off, the other half's [0, hv2) becomes sequence
 *                          samples [drop, drop + hv2); the arithmetic is wv_native_session_down's for that stream.
 *   wv_native_bank_up_add  desc [P][15] = {slot, rate, C, rv, r_off, nr, x_off, n, out_off, k, pad, rdrop, rv2, pv, half}, gain [P] f32 on the device
 *                          (row p's strength): the row's nr residual samples lie at r + r_off, its new originals (C x n) at x + x_off, and its output,
 *                          C planar channels of k floats, goes to out + out_off, formed as wv_native_session_up_add forms it; the next residual
 *                          history [0, rv2) and the next delay line [c][0, pv2), pv2 = pv + n - k, go to the other half.
 * `blocks` is the launch's x-extent, which the entry point cannot read from device descriptors: at least the largest per-row need, which is
 * ceil(n_out / 256) + ceil(hv2 / 256) for the front stage and ceil(k / 256) + ceil(rv2 / 256) + ceil(pv2 / 256) for the back stage.  Blocks past
 * a row's own need exit; a row that needs more than `blocks` is served only in part.
 * ROW RULE (native_bank.native_bank_down_row_ok / native_bank_up_row_ok state it in Python): a row is served only if
 *   0 <= slot < capacity, 0 <= rate < n_rates, 1 <= C <= 64 (and C <= Cmax for the back stage), half in {0, 1};
 *   each rolled state is a fitting suffix: 0 <= valid <= cap, 0 <= next <= cap, fresh >= 0, drop >= 0, drop + next == valid + fresh, for
 *   (hcap, hv, n, drop, hv2) and (rcap, rv, nr, rdrop, rv2);  0 <= pv <= pcap, n >= 0, k >= 0, 0 <= pv + n - k <= pcap;
 *   0 <= pad <= the rate's width;  0 <= outputs <= (ceil((pad + valid + fresh) / orig) + 1) * nw;  every sample count <= 2^31 - 257;
 *   every range inside its arena: x_off >= 0 and x_off + C * n <= n_x, and likewise y_off + n_out <= n_y, r_off + nr <= n_r, out_off + C * k <= n_out.
 * Any other row is skipped WHOLE: none of its outputs is written and both halves of its slot stay untouched; the other rows of the call are served.
 * Refused with WV_EINVAL, nothing launched or written: a null pointer where a count is positive (hist, rhist, pend and rates always; desc and gain
 * with P > 0), capacity outside [1, WV_BANK_MAX_SLOTS], P outside [0, 65535], blocks outside [0, WV_NATIVE_BANK_MAX_BLOCKS], n_rates outside
 * [1, WV_NATIVE_BANK_MAX_RATES], a rate entry with orig, nw or L < 1, width < 0 or a null table, hcap, rcap or pcap < 1, Cmax outside [1, 64], a
 * negative arena length, or arenas that overlap each other or the state buffers (r and x, both only read, may).  P == 0 or blocks == 0 is success
 * without a launch. */
#define WV_NATIVE_BANK_MAX_RATES 8
#define WV_NATIVE_BANK_MAX_BLOCKS 16777216
typedef struct { const float* kernels_t; int orig, nw, L, width; } wv_native_rate;
int wv_native_bank_down(float* hist, int capacity, int hcap, const float* x, int64_t n_x, const wv_native_rate* rates, int n_rates, const int64_t* desc,
                        int P, int blocks, float* y, int64_t n_y, void* stream);
int wv_native_bank_up_add(float* rhist, int rcap, float* pend, int pcap, int Cmax, int capacity, const float* r, int64_t n_r, const float* x, int64_t n_x,
                          const wv_native_rate* rates, int n_rates, const int64_t* desc, const float* gain, int P, int blocks, float* out, int64_t n_out,
                          void* stream);

/* ---- csrc/wv_live_floor.hip: wv_native_bank_up_add under the PER-CHANNEL SNR floor (native_bank.numpy_bank_floor_up_add
 * restates it, row rule included): per stream the concatenated output is wv_native_floor_up_add's arithmetic (channel_floor.numpy_channel_floor) on
 * everything the stream pushed, bit for bit.  A sample leaves only when its whole native frame has its u, so besides rhist and pend a slot keeps
 *   uhold [capacity][2][ucap]  the u already formed for samples not yet emitted (fewer than one frame), and
 *   gprev [capacity][2][Cmax]  the gains of the last frame emitted, per channel,
 * ping-pong like the others.  With seq_u = cat(uhold[0 .. uv), new u) and seq_x[c] = cat(pend[c][0 .. pv), x[c][0 .. n)), both beginning at the
 * stream's first sample not yet emitted, start(f0), start(f) = ceil(f * nw * hop / orig):
 *   desc [P][21] = {slot, rate, C, rv, r_off, nr, x_off, n, out_off, k, pad, rdrop, rv2, pv, half, f0, nf, uv, uv2, g_off, final}: the first fifteen
 *     are wv_native_bank_up_add's, except that k counts the samples that LEAVE; the chain forms k + uv2 - uv new u.  Frames f0 .. f0 + nf - 1 complete:
 *     their Eu and Ex[c] come from seq_u and seq_x in wv_snr_floor's fixed order, the gains follow wv_native_floor_up_add's rule with cap[p] (f32,
 *     DEVICE) as the cap s and rho, the gain before frame f0 is gprev (the stream's frame 0 takes its own gain and reads no state), and
 *     out[c][i] = seq_x[c][i] + w * seq_u[i], i < k, with seq_x's own bits where w * seq_u[i] is +0 or -0: C planar channels of k floats at
 *     out + out_off.  The other half takes rhist's next samples, seq_x[c][k .. k + pv2), seq_u[k .. k + uv2) and the gains of frame f0 + nf - 1
 *     (nf == 0: gprev as it was).  g_off >= 0: the gains go to gains + g_off as [C][nf] as well; -1: nowhere.  final: the stream's last call, whose
 *     last frame is cut at k with its nominal length in the ramp.
 * One launch.  `blocks` is at least the largest per-row need, ceil(nf / NF) + ceil(rv2 / 256) + ceil(pv2 / 256) + ceil(uv2 / 256) + (nf == 0), NF the
 * rate's frames per workgroup (native_bank.floor_tile_frames).
 * ROW RULE: wv_native_bank_up_add's with k + uv2 - uv as the outputs of the chain, and 0 <= uv, uv2 <= ucap; final in {0, 1} and uv2 == 0 where it is
 * set; k + uv2 - uv >= 0; f0 >= 0, 0 <= nf <= 2^31 - 257, f0 + nf <= 2^62 / (nw * hop); k == start(f0 + nf) - start(f0), at final instead
 * start(f0 + nf - 1) - start(f0) < k <= start(f0 + nf) - start(f0) (nf == 0: k == 0); g_off == -1, or g_off >= 0 and g_off + C * nf <= n_gains;
 * cap[p] finite and >= 0.  Any other row is skipped WHOLE: no output, no gains, both halves of all four states untouched.
 * Refused with WV_EINVAL, nothing launched or written: everything wv_native_bank_up_add refuses; null uhold or gprev, gains null with n_gains > 0;
 * ucap < 1, n_gains < 0, hop < 1, rho not finite or <= 0; a rate with nw * hop beyond 2^31 - 1, a frame of ceil(nw * hop / orig) >
 * WV_CHANNEL_FLOOR_MAX_FRAME native samples, or TWO such frames (a workgroup also holds the frame before its own) that with the 256-output input
 * window and 1088 floats of gains pass WV_CHANNEL_FLOOR_LDS_FLOATS; states or arenas that overlap (r and x may).  P == 0 or blocks == 0 is success
 * without a launch. */
int wv_native_bank_floor_up_add(float* rhist, int rcap, float* pend, int pcap, float* uhold, int ucap, float* gprev, int Cmax, int capacity,
                                const float* r, int64_t n_r, const float* x, int64_t n_x, const wv_native_rate* rates, int n_rates, const int64_t* desc,
                                const float* cap, int P, int blocks, int hop, double rho, float* out, int64_t n_out, float* gains, int64_t n_gains,
                                void* stream);

/* ==== csrc/wv_fx_time.hip: plain-arithmetic time-domain effects ----------------------------------------------------------------
 * The reference's remaining AudioEffects that are arithmetic of its own (utils/effect_augmentation.py:1081-1332,1504-1681,1873-2132,
 * 2338-2404): PINNED to the reference by tests/golden/effects_time.npz, bit for bit where the result is a selection or one rounding
 * per sample, to 2e-5 of the peak where it is a float sum.  Device pointers, [rows][T] contiguous f32, rows <= 65535, rows * T < 2^32;
 * any alignment of 4 bytes is accepted.  The random draws are made on the host (waveverify_amd/effects.py) and arrive as arguments. */
/* pointwise pass, one rounding per operation in the reference's order (the library is built without contraction):
 *   WV_FX_SCALE      y = x * a                          (amplitude_scaling)
 *   WV_FX_ADD_NOISE  y = x + noise * a                  (random_noise / white_noise / pink_noise; noise [rows][T])
 *   WV_FX_QUANTIZE   y = rint(x * a) / a, a = 2^(bits-1) - 1, half to even, IEEE divide (a = 0 gives NaN, as the reference does for 1 bit)
 *   WV_FX_MUL        y = x * noise                      (shush's backward: gradient * keep mask; a is ignored)
 * noise may be NULL for the two one-tensor ops. */
#define WV_FX_SCALE 0
#define WV_FX_ADD_NOISE 1
#define WV_FX_QUANTIZE 2
#define WV_FX_MUL 3
int wv_fx_pointwise(const float* x, const float* noise, float* y, int rows, int T, int op, float a, void* stream);
/* scipy.signal.medfilt: y[t] = median of x[t - k/2 .. t + k/2] with ZEROS outside [0, T); k odd.  k <= WV_FX_MEDIAN_NET_K sorts the
 * window in registers, larger k up to WV_FX_MEDIAN_MAX_K counts ranks over the LDS tile (O(k^2) per sample); any other k is refused.
 * A NaN in a window is outside the contract. */
#define WV_FX_MEDIAN_NET_K 31
#define WV_FX_MEDIAN_MAX_K 255
int wv_fx_median(const float* x, float* y, int rows, int T, int k, void* stream);
/* shush: per row, zero exactly k (0 <= k <= T - 1) samples: every sample whose |x| is below the k-th smallest, and the earliest ones
 * equal to it until k are gone (torch.topk leaves the choice among equals open; this one is deterministic).  y = x * keep,
 * keep [rows][T] = 0 / 1 (the backward's mask), and with mask_in: mask_out = mask_in * (y != 0) -- samples that were 0 already clear
 * the mask too.  k = 0 copies.  mask_in / mask_out may both be NULL. */
int wv_fx_shush(const float* x, const float* mask_in, float* y, float* keep, float* mask_out, int rows, int T, int k, void* stream);
/* echo: c[r][t] = x[r][t] + volume * x[r][t + n - 1] for t < T - n + 1 (cross-correlation with [1, 0, .., 0, volume], n taps, 2 <= n <= T:
 * the delayed copy comes BEFORE the sound, as in the reference), y = c / max|c| * max|x| with both maxima over the WHOLE tensor and only
 * when both are > 0; the last n - 1 samples of each row are 0.  Two launches: the peaks call fills the record (WV_FX_ECHO_RECORD_BYTES,
 * 8-byte aligned: two 64-bit words, (bits of the maximum) << 32 | ~(flat position), for x then for c), the apply call reads it.
 * The backward is the reference's autograd through the correlation and both maxima; it needs x, the record of the forward and a
 * workspace of wv_fx_echo_backward_workspace_bytes() (any contents: partial sums of g * c and partial counts of the tied peaks),
 * and sums g * c in a fixed order.  Ties for a maximum are inside the contract: the forward does not depend on which of several equal
 * peaks is recorded (the earliest), and the backward shares each maximum's gradient evenly among ALL positions whose magnitude equals
 * it, as torch's autograd of a full-reduction max does (clipped audio has many); it reads only the magnitudes of the record, not the
 * positions.  With one peak each the result is that of the recorded positions. */
#define WV_FX_ECHO_RECORD_BYTES 16
int wv_fx_echo_peaks(const float* x, void* rec, int rows, int T, int n, float volume, void* stream);
int wv_fx_echo_apply(const float* x, const void* rec, float* y, int rows, int T, int n, float volume, void* stream);
size_t wv_fx_echo_backward_workspace_bytes(void);
int wv_fx_echo_backward(const float* x, const float* g, const void* rec, float* dx, int rows, int T, int n, float volume, void* workspace,
                        size_t workspace_bytes, void* stream);
/* smooth: y[t] = sum_j xpad[t + j] / w over w taps, xpad = x REFLECT-padded by pad_l = (w-1)/2 in front and pad_r = w-1-pad_l behind
 * (pad_r < T, w <= WV_FX_SMOOTH_MAX_W); with mask_in: mask_out[t] = (count / w >= valid_threshold) in f32, count = the window sum of the
 * ZERO-padded mask.  The backward is the transposed box filter followed by the transpose of the reflect padding, in one kernel. */
#define WV_FX_SMOOTH_MAX_W 2048
int wv_fx_smooth(const float* x, const float* mask_in, float* y, float* mask_out, int rows, int T, int w, float valid_threshold, void* stream);
int wv_fx_smooth_backward(const float* g, float* dx, int rows, int T, int w, void* stream);
/* y[r][idx[r][j]] = 0 for j < num, in place, and the same on mask when it is not NULL; idx [rows][num] int32, entries outside [0, T) are
 * skipped.  sample_suppression's forward (on a copy of the input) and, on the gradient, its backward. */
int wv_fx_scatter_zero(float* y, float* mask, const int* idx, int rows, int T, int num, void* stream);
/* torch.nn.functional.interpolate(mode='linear', align_corners=False) from Tin to Tout samples: source coordinate
 * max(0, (m + 0.5) * Tin / Tout - 0.5) with the scale in f32 and the multiply-add rounded once (fused), as torch's CPU kernel
 * evaluates it (AudioProcessor.adjust_audio_length(mode='stretch')); i0 = min(int(coordinate), Tin - 1), the blend in f32. */
int wv_fx_stretch_linear(const float* x, float* y, int rows, int Tin, int Tout, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* WAVEVERIFY_HIP_H */
