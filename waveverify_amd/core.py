"""WaveVerify: the reference's package API on the MI355X-native path.

Same constructor, methods, return types and error wrapping as
/root/reference/waveverify/core.py:51-729 — `WaveVerify(checkpoint, device)`,
`.embed/.detect/.locate/.verify` — plus batched tensor entry points (`embed_batch`,
`detect_batch`, `locate_batch`) that the file-based methods are thin wrappers of.  The forward
passes run in libwaveverify_hip.so (see nets.py); there is no CPU fallback.
"""
from __future__ import annotations

import logging
import math
from pathlib import Path
from types import SimpleNamespace
from typing import Dict, List, Mapping, Optional, Tuple, Union

import numpy as np
import torch

from . import localize, native, native_bank, native_session, ops, session, snr_floor, window
from .checkpoint import load_checkpoint
from .config import NetConfig, default_config
from .init import random_state_dict
from .localize import Segment
from .nets import HipNet
from .utils import load_audio, load_audio_native, message_to_tensor, save_audio, tensor_to_message
from .watermark_id import WatermarkID

logger = logging.getLogger(__name__)

# the live per-channel floor holds output until each native frame completes: a bank of its own opener has it, the
# lockstep sessions, which have no 16 kHz floor either, do not
_NO_LIVE_CHANNEL_FLOOR = ("open_embed_bank(rates=...) and the lockstep native-rate embed sessions have no per-channel SNR floor: open the bank "
                          "with open_native_embed_bank (DESIGN.md section 7d-13), embed files with embed(native=True) / embed_native_batch, or "
                          "call set_channel_snr_floor(None) first")


class WaveVerify:
    DEFAULT_SAMPLE_RATE: int = 16000
    DEFAULT_WATERMARK_BITS: int = 16
    # NOT in the reference: the SNR floor of embedding in dB (set_snr_floor).  None runs nothing new.
    snr_floor_db: Optional[float] = None
    # NOT in the reference: the per-channel floor of the native-rate file routes (set_channel_snr_floor) and of
    # open_native_embed_bank (section 7d-13).
    channel_snr_floor_db: Optional[float] = None

    def __init__(self, checkpoint: Union[str, Path, Mapping] = "base", device: str = "auto") -> None:
        """checkpoint: "base" (the reference's download URL is empty upstream, utils.py:45-52, so
        this fails exactly as it does there), a path to an atomic .pth / checkpoint directory /
        legacy directory, or a mapping {"generator"|"detector"|"locator": state_dict}."""
        try:
            self.device = self._setup_device(device)
            if isinstance(checkpoint, Mapping):
                sds = {k: dict(v) for k, v in checkpoint.items()}
                from .checkpoint import infer_config
                cfgs = {k: infer_config(k, sd) for k, sd in sds.items()}
            else:
                if checkpoint == "base":
                    raise FileNotFoundError(
                        "the pre-trained 'base' checkpoint is not distributed (empty download URL in the "
                        "reference, waveverify/utils.py:45-52); pass a checkpoint path")
                sds, cfgs = load_checkpoint(Path(checkpoint))
            self._build(sds, cfgs)
            self.sample_rate = self.DEFAULT_SAMPLE_RATE
            self.watermark_bits = self.DEFAULT_WATERMARK_BITS
        except Exception as e:
            logger.error(f"Failed to initialize WaveVerify: {str(e)}")
            raise RuntimeError(f"WaveVerify initialization failed: {str(e)}") from e

    @classmethod
    def random_init(cls, seed: int = 0, device: str = "auto",
                    configs: Optional[Dict[str, NetConfig]] = None) -> "WaveVerify":
        """Seeded random weights (benchmarks, tests): no trained checkpoint ships upstream."""
        cfgs = configs or {k: default_config(k) for k in ("generator", "detector", "locator")}
        self = cls.__new__(cls)
        self.device = self._setup_device(device)
        self._build({k: random_state_dict(c, seed) for k, c in cfgs.items()}, cfgs)
        self.sample_rate, self.watermark_bits = cls.DEFAULT_SAMPLE_RATE, cls.DEFAULT_WATERMARK_BITS
        return self

    def _build(self, sds, cfgs) -> None:
        nets = {k: HipNet(cfgs[k], sds[k], self.device) for k in sds}
        self.configs = cfgs
        # NOT in the reference: "f16" routes detect / detect_batch / verify through the detector's f16-operand / f32-accumulate mode
        # (csrc/wv_h16.hip; the same bits on every fixture, ~3x the clips per second).  Opt-in only; the default is the exact path.
        self.detector_precision = "f32"
        # ... and the same switch for embed / embed_batch (`wm` stays within 1e-4 of the exact path's and the reference's) and locate /
        # locate_batch.  `set_precision("f16")` flips all three; `value` of the headline benchmark is always the exact path.
        self.generator_precision = "f32"
        self.locator_precision = "f32"
        # .model.generator / .detector / .locator like the reference's AudioWatermarking
        self.model = SimpleNamespace(generator=nets.get("generator"), detector=nets.get("detector"),
                                     locator=nets.get("locator"))

    def _setup_device(self, device: str) -> torch.device:
        if device == "auto":
            if not torch.cuda.is_available():
                raise RuntimeError("no MI355X visible and waveverify_amd has no CPU path")
            return torch.device("cuda", torch.cuda.current_device())
        return torch.device(device)

    def set_precision(self, precision: str) -> None:
        """NOT in the reference: "f32" (default, exact) or "f16" (the f16-operand / f32-accumulate throughput mode) for all three nets."""
        if precision not in ("f32", "f16"):
            raise ValueError("precision must be 'f32' or 'f16'")
        self.generator_precision = self.detector_precision = self.locator_precision = precision

    def set_snr_floor(self, min_snr_db: Optional[float]) -> None:
        """NOT in the reference: with a number, every embed route scales the generator's residual frame by frame (frames of the generator's
        hop at 16 kHz) so that in no frame the watermark is louder than min_snr_db below the programme, and silence stays silent
        (snr_floor.py).  None (the default) switches it off.  The floor is defined on the 16 kHz mono time
        line; at a native rate it does not bound the SNR of a channel: set_channel_snr_floor does."""
        self.snr_floor_db = snr_floor.check_db(min_snr_db)

    def set_channel_snr_floor(self, min_snr_db: Optional[float]) -> None:
        """NOT in the reference: with a number, the native-rate file routes (embed_native_batch, embed_spans_native_batch, embed and
        embed_spans with native=True) hold the floor on every ORIGINAL channel at the file's own rate: in no native frame of any channel
        is the watermark louder than min_snr_db below that channel, and a silent channel comes back bit for bit (channel_floor.py,
        native.upsample_add_floor).  None (the default) switches it off.  The 16 kHz routes are not touched:
        their one mono channel is set_snr_floor's.  With both floors set the 16 kHz floor shapes the residual first, `strength` inside
        it, and the channel floor runs on that residual with cap 1.0; alone, `strength` is the channel floor's cap.  The live native
        routes (open_embed_session with a rate, open_embed_bank(rates=...)) have no channel floor and refuse to open under one."""
        self.channel_snr_floor_db = snr_floor.check_db(min_snr_db)

    def _native_back_end(self, audio, delta, sample_rate: int, strength):
        """The last step of the native-rate file routes: delta onto every channel, under the channel floor where one is set."""
        if self.channel_snr_floor_db is None:
            return native.upsample_add(audio, delta, sample_rate, strength)
        return native.upsample_add_floor(audio, delta, sample_rate, self.channel_snr_floor_db, strength,
                                         hop=self._need("generator").hop_length)

    def _floor(self, x, residual, strength=1.0, add: bool = True):
        """The floor on a 16 kHz input and its residual, frames of the generator's hop."""
        return snr_floor.apply(x, residual, self.snr_floor_db, strength, frame=self._need("generator").hop_length, add=add)

    def _need(self, name: str) -> HipNet:
        net = getattr(self.model, name)
        if net is None:
            raise RuntimeError(f"checkpoint holds no {name} weights")
        return net

    # ------------------------------------------------------------------ batched tensor API
    @torch.no_grad()
    def embed_batch(self, audio: torch.Tensor, message: torch.Tensor) -> torch.Tensor:
        """audio [B,1,T] (or [B,T]); message [B,16] or [1,16] (0/1) -> watermarked [B,1,T]."""
        gen = self._need("generator")
        if self.snr_floor_db is None:
            return gen.generator(audio, message, add_input=True, precision=self.generator_precision)
        x = gen._prep(audio)
        return self._floor(x, gen.generator(x, message, add_input=False, precision=self.generator_precision))

    @torch.no_grad()
    def detect_batch(self, audio: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
        """-> (bits [B,16] int32, mean_prob [B,16]); bits = time-averaged sigmoid >= 0.5."""
        mp = self._need("detector").detector_mean_prob(audio, precision=self.detector_precision)
        return (mp >= 0.5).to(torch.int32), mp

    @torch.no_grad()
    def locate_batch(self, audio: torch.Tensor) -> torch.Tensor:
        """-> sigmoid(locator logits) [B, T]."""
        return torch.sigmoid(self._need("locator").locator(audio, precision=self.locator_precision)).squeeze(1)

    # ------------------------------------------------------------------ native rate and channel count (NOT in the reference)
    @torch.no_grad()
    def to_model_rate(self, audio: torch.Tensor, sample_rate: int) -> torch.Tensor:
        """audio [B,C,Tn] (or [C,Tn]) at `sample_rate` -> the model's input [B,1,T16]: the channel mean at 16 kHz, one kernel
        (native.downmix_resample).  For one or two channels these are the bits load_audio gives for the same file."""
        return native.downmix_resample(audio.to(self.device), sample_rate)

    @torch.no_grad()
    def embed_native_batch(self, audio: torch.Tensor, sample_rate: int, message: torch.Tensor, strength: float = 1.0,
                           window_seconds: Optional[float] = None) -> torch.Tensor:
        """audio [B,C,Tn] (or [C,Tn]) at `sample_rate`; message [B,16] or [1,16] -> watermarked [B,C,Tn] at the same rate: the generator
        runs on to_model_rate(audio), its residual alone is resampled back to `sample_rate` and strength times it is added to every
        channel (native.upsample_add).  window_seconds: run the 16 kHz copy as windows of that length.  What a detector later sees is
        x16 + down(up(residual)), not x16 + residual: DESIGN.md section 7d-3."""
        gen = self._need("generator")
        audio = audio.to(self.device)
        x16 = self.to_model_rate(audio, sample_rate)
        if window_seconds is None:
            delta = gen.generator(x16, message, add_input=False, precision=self.generator_precision)
        else:
            delta = window.windowed_generator(gen, x16, message, self._window_samples(window_seconds), self.generator_precision, add_input=False)
        if self.snr_floor_db is not None:                                  # the strength moves into the floor
            return self._native_back_end(audio, self._floor(x16, delta, strength, add=False), sample_rate, 1.0)
        return self._native_back_end(audio, delta, sample_rate, strength)

    # ------------------------------------------------------------------ localized detection (NOT in the reference's package API)
    def _gate(self, audio, threshold: float, gate):
        """-> (gate tensor, gate_thr) for the frames kernels: a caller's 0/1 mask with 0.5, else the locator's LOGITS with the logit of
        `threshold` (sigmoid(logit) > threshold, strict, without writing a gate tensor of its own)."""
        if gate is not None:
            return gate, 0.5
        return self._need("locator").locator(audio, precision=self.locator_precision), localize.gate_threshold(threshold)

    def _segments(self, fsum, lengths, hop: int, min_on: float, min_gap_frames: int, min_len_frames: int) -> List[List[Segment]]:
        """Per-clip frame sums (a list of [nb + 1, Fr_b], or [B, nb + 1, Fr]) -> per clip its Segments: runs of on frames from the count
        row, then ONE wv_frames_reduce over all of them."""
        per_clip = list(fsum) if not isinstance(fsum, torch.Tensor) else [fsum[b] for b in range(fsum.shape[0])]
        nb = per_clip[0].shape[0] - 1
        Frs = [int(f.shape[1]) for f in per_clip]
        stride = max(Frs)
        flat = torch.zeros((len(per_clip), nb + 1, stride), dtype=torch.float32, device=per_clip[0].device)
        for b, f in enumerate(per_clip):
            flat[b, :, :Frs[b]] = f
        counts = flat[:, nb, :].cpu().numpy()
        segs = []
        for b, T in enumerate(lengths):
            for lo, hi in localize.segments_from_counts(counts[b, :Frs[b]], localize.frame_valid(T, hop), min_on, min_gap_frames, min_len_frames):
                segs.append((b, lo, hi))
        out: List[List[Segment]] = [[] for _ in lengths]
        if not segs:
            return out
        prob, count = ops.frames_reduce(flat, segs)
        prob, count = prob.cpu(), count.cpu().numpy()
        for i, (b, lo, hi) in enumerate(segs):
            n = min(hi * hop, lengths[b]) - lo * hop
            out[b].append(Segment(lo * hop / self.sample_rate, min(hi * hop, lengths[b]) / self.sample_rate,
                                  WatermarkID.custom(tensor_to_message(prob[i])), float(prob[i].mean()), float(count[i]) / n,
                                  prob[i].numpy(), (lo, hi)))
        return out

    def _segments_split(self, fsum, lengths, hop: int, min_on: float, min_gap_frames: int, min_len_frames: int, split) -> List[List[Segment]]:
        """_segments under a localize.SplitRule: the clips' frame sums stay on the device and go through ONE wv_bank_segment_track_split
        launch, a descriptor per clip {clip, offset of its rows, row length, 0, its frames, 0, the last frame's samples, final}; only the
        event records in use come back (the counters are read first)."""
        per_clip = list(fsum) if not isinstance(fsum, torch.Tensor) else None
        B = len(per_clip) if per_clip is not None else fsum.shape[0]
        nb = (per_clip[0] if per_clip is not None else fsum).shape[-2] - 1
        split.check(nb, min_gap_frames, min_len_frames)
        Frs = [int(f.shape[1]) for f in per_clip] if per_clip is not None else [int(fsum.shape[2])] * B
        arena = torch.cat([f.float().reshape(-1) for f in per_clip]) if per_clip is not None else fsum.float().contiguous().reshape(-1)
        desc, off = [], 0
        for b, (Fr, T) in enumerate(zip(Frs, lengths)):
            desc.append([b, off, Fr, 0, Fr, 0, int(T) - (Fr - 1) * hop, 1])
            off += (nb + 1) * Fr
        # events are disjoint stretches of frames: a piece of a cut run has at least window_frames, an uncut run at least
        # max(1, min_len_frames) and min_gap_frames off frames behind it (but for a clip's last)
        ring = max(Frs) // min(split.window_frames, max(1, min_len_frames) + min_gap_frames) + 1
        dev = arena.device
        with torch.cuda.device(dev):
            sb, eb = ops.segment_split_bytes(B, nb, min_gap_frames, split.window_frames, ring)
            state = torch.zeros(sb, dtype=torch.uint8, device=dev)
            events = torch.zeros(eb, dtype=torch.uint8, device=dev)
            ops.bank_segment_track_split(arena, torch.tensor(desc, dtype=torch.int64).to(dev), B, B, nb, hop, min_on, min_gap_frames,
                                         min_len_frames, split, state, events, ring)
            rows = events.view(B, -1)
            n = rows[:, :8].contiguous().cpu().numpy().view("<i8").reshape(B)      # the counters first, then only the records in use
            used = ops.split_event_dtype(nb).itemsize * int(n.max()) if B else 0
            recs = rows[:, 8:8 + used].contiguous().cpu().numpy().view(ops.split_event_dtype(nb)).reshape(B, -1)
        out: List[List[Segment]] = [[] for _ in lengths]
        for b, T in enumerate(lengths):
            for r in recs[b, :int(n[b])]:
                lo, hi, prob = int(r["lo"]), int(r["hi"]), torch.from_numpy(r["prob"].copy())
                end = min(hi * hop, int(T))
                wid = WatermarkID.custom(tensor_to_message(prob)) if nb == 16 else None     # an id has 16 bits; another width leaves prob to read
                out[b].append(Segment(lo * hop / self.sample_rate, end / self.sample_rate, wid, float(prob.mean()),
                                      float(r["count"]) / (end - lo * hop), prob.numpy(), (lo, hi), (bool(r["flags"] & 1), bool(r["flags"] & 2))))
        return out

    @torch.no_grad()
    def detect_localized_batch(self, audio: torch.Tensor, threshold: float = 0.5,
                               gate: Optional[torch.Tensor] = None) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
        """Decode only where the watermark is: -> (bits [B,16] int32, prob [B,16], coverage [B] float64).  prob is the mean of
        sigmoid(detector logit) over the samples the locator marks (sigmoid(locator logit) > threshold), the reference's masked BER
        decode (scripts/evaluate.py:442-516), without storing any logits; bits = prob >= 0.5; coverage = marked samples / T.
        gate [B,T] (0/1) replaces the locator.  A clip with coverage 0 has no watermark found: its prob and bits are 0."""
        det = self._need("detector")
        g, thr = self._gate(audio, threshold, gate)
        fsum = det.detector_frame_sums(audio, g, thr, self.detector_precision)
        B, _, Fr = fsum.shape
        prob, count = ops.frames_reduce(fsum, [(b, 0, Fr) for b in range(B)])
        return (prob >= 0.5).to(torch.int32), prob, count / torch.full_like(count, float(audio.shape[-1]))   # a true division, element by element

    @torch.no_grad()
    def detect_segments_batch(self, audio: torch.Tensor, threshold: float = 0.5, gate: Optional[torch.Tensor] = None, min_on: float = 0.5,
                              min_gap_frames: int = 2, min_len_frames: int = 5, split=None) -> List[List[Segment]]:
        """Per clip the list of watermarked Segments (localize.segments_from_counts on the gated sample counts per detector frame), each
        decoded over its own gated samples: a clip spliced from differently marked sources gives one Segment per source.
        split: a localize.SplitRule; a run is then also cut where the decoded id changes inside it (abutting stretches marked with
        different ids), each Segment's `change` saying which of its ends is such a cut."""
        det = self._need("detector")
        g, thr = self._gate(audio, threshold, gate)
        fsum = det.detector_frame_sums(audio, g, thr, self.detector_precision)
        lengths = [int(audio.shape[-1])] * fsum.shape[0]
        if split is not None:
            return self._segments_split(fsum, lengths, det.hop_length, min_on, min_gap_frames, min_len_frames, split)
        return self._segments(fsum, lengths, det.hop_length, min_on, min_gap_frames, min_len_frames)

    # ------------------------------------------------------------------ windowed: variable-length clips, live sessions (NOT in the reference)
    def _window_samples(self, window_seconds: float) -> int:
        """window_seconds -> samples, rounded up to the lcm of the nets' hops so one plan suits embed, detect and locate."""
        if not window_seconds or window_seconds <= 0:
            raise ValueError("window_seconds must be positive")
        hop = window.pipeline_hop([c for c in self.configs.values()])
        return -(-int(math.ceil(window_seconds * self.sample_rate)) // hop) * hop

    def _messages(self, watermark_ids) -> torch.Tensor:
        if isinstance(watermark_ids, (list, tuple)):
            ids = [self._validate_watermark_id(w) for w in watermark_ids]
        else:
            ids = [self._validate_watermark_id(watermark_ids)]
        return torch.cat([message_to_tensor(w.to_bits(), self.watermark_bits) for w in ids]).to(self.device)

    @torch.no_grad()
    def embed_clips(self, clips, watermark_ids, window_seconds: float = 30.0):
        """clips: a list of 1-D tensors of any lengths (or [B,1,T]); watermark_ids: one per clip, or one for all
        -> the watermarked clips, same kind as `clips`.  Long clips run as windows (window.py)."""
        if self.snr_floor_db is not None:
            clips = self._on_device(clips)
            return self._floor(clips, window.windowed_generator(self._need("generator"), clips, self._messages(watermark_ids),
                                                                self._window_samples(window_seconds), self.generator_precision, add_input=False))
        return window.windowed_generator(self._need("generator"), clips, self._messages(watermark_ids),
                                         self._window_samples(window_seconds), self.generator_precision)

    def _on_device(self, clips):
        """clips ([B,1,T] or a list of 1-D tensors) as float32 on the device, the same kind."""
        if isinstance(clips, torch.Tensor):
            return clips.to(self.device, torch.float32)
        return [c.to(self.device, torch.float32) for c in clips]

    # ------------------------------------------------------------------ span embedding (NOT in the reference)
    def _span_messages(self, spans):
        """Per clip a list of (start, end, watermark id) -> (messages [M,16] of the distinct ids, the spans with each id replaced by its
        row, the validated ids in the spans' order)."""
        rows, ids, out = {}, [], []
        for lst in spans:
            mine = []
            for s, e, w in lst:
                w = self._validate_watermark_id(w)
                ids.append(w)
                mine.append((s, e, rows.setdefault(w.to_bits(), len(rows))))
            out.append(mine)
        if not rows:
            return torch.zeros((1, self.watermark_bits)), out, ids
        return torch.cat([message_to_tensor(bits, self.watermark_bits) for bits in rows]), out, ids

    @torch.no_grad()
    def embed_spans_clips(self, clips, spans, window_seconds: float = 30.0, fade_samples: int = 0, strength: float = 1.0,
                          pad_limit: float = 1.5):
        """Watermark chosen stretches, each with its own id.  clips: a list of 1-D tensors of any lengths (or [B,1,T]); spans: per clip a
        list of (start, end, watermark_id) in samples, disjoint (abutting is allowed) -> the clips, same kind: inside a span
        x + w * G(x, id)'s residual of the whole clip, w = strength times a raised-cosine ramp of fade_samples at both span edges
        (0: a hard cut); outside every span the input bit for bit.  Only halo + span samples go through the generator."""
        msgs, rows, _ = self._span_messages(spans)
        if self.snr_floor_db is not None:                                  # the masked residual (span weights and strength inside), then the floor
            clips = self._on_device(clips)
            return self._floor(clips, window.span_generator(self._need("generator"), clips, msgs, rows, self._window_samples(window_seconds),
                                                            self.generator_precision, pad_limit, fade_samples=fade_samples, gain=strength,
                                                            add_input=False))
        return window.span_generator(self._need("generator"), clips, msgs, rows, self._window_samples(window_seconds), self.generator_precision,
                                     pad_limit, fade_samples=fade_samples, gain=strength)

    @torch.no_grad()
    def embed_spans_native_batch(self, audio: torch.Tensor, sample_rate: int, spans, strength: float = 1.0, fade_samples: int = 0,
                                 window_seconds: float = 30.0) -> torch.Tensor:
        """embed_native_batch for chosen stretches: audio [B,C,Tn] (or [C,Tn]) at `sample_rate`; spans per clip (start, end, watermark_id) in
        16 kHz samples of to_model_rate(audio), fade_samples too.  The masked residual is built dense at 16 kHz (zeros outside the spans),
        then brought up to `sample_rate` and added to every channel by the one full-length native.upsample_add pass."""
        gen = self._need("generator")
        audio = audio.to(self.device)
        msgs, rows, _ = self._span_messages(spans)
        x16 = self.to_model_rate(audio, sample_rate)
        if self.snr_floor_db is not None:                                  # the strength moves into the masked residual, under the floor
            d16 = window.span_generator(gen, x16, msgs, rows, self._window_samples(window_seconds), self.generator_precision,
                                        fade_samples=fade_samples, gain=strength, add_input=False)
            return self._native_back_end(audio, self._floor(x16, d16, add=False), sample_rate, 1.0)
        d16 = window.span_generator(gen, x16, msgs, rows, self._window_samples(window_seconds), self.generator_precision,
                                    fade_samples=fade_samples, gain=1.0, add_input=False)
        return self._native_back_end(audio, d16, sample_rate, strength)

    def embed_spans(self, audio_path: Union[str, Path], spans, output_path: Optional[Union[str, Path]] = None, *, native: bool = False,
                    strength: float = 1.0, fade_ms: float = 0.0, window_seconds: float = 30.0) -> Tuple[np.ndarray, int, List[WatermarkID]]:
        """embed for chosen stretches of a file: spans (start_s, end_s, watermark_id) in seconds, rounded to 16 kHz samples; an end past the
        file's end is clamped -> (array, sample rate, the validated ids) shaped as embed's.  native, strength: as in embed."""
        if not native and strength != 1.0:
            raise ValueError("strength other than 1.0 needs native=True (the reference's route adds the residual as it is)")
        try:
            fs = self.sample_rate
            fade = int(round(float(fade_ms) * fs / 1000.0))
            in_samples = lambda T: [[(int(round(float(s) * fs)), min(int(round(float(e) * fs)), T), w) for s, e, w in spans]]   # noqa: E731
            ids = [self._validate_watermark_id(w) for _, _, w in spans]
            if native:
                audio, sr = load_audio_native(audio_path)                           # [C, Tn] at the file's rate
                T16 = int(self.to_model_rate(audio.unsqueeze(0), sr).shape[-1])
                wm = self.embed_spans_native_batch(audio.unsqueeze(0), sr, in_samples(T16), strength, fade, window_seconds).squeeze(0)
                if output_path:
                    save_audio(wm, output_path, sr)
                out = wm.cpu().numpy()
                return (out[0] if out.shape[0] == 1 else out), sr, ids
            audio, _ = load_audio(audio_path, fs)
            wm = self.embed_spans_clips(audio.unsqueeze(0), in_samples(int(audio.shape[-1])), window_seconds, fade).squeeze(0)
            if output_path:
                save_audio(wm, output_path, fs)
            return wm.cpu().numpy().squeeze(), fs, ids
        except Exception as e:
            logger.error(f"Span embedding failed: {str(e)}")
            raise RuntimeError(f"Failed to embed watermark spans: {str(e)}") from e

    def _clip_frame_sums(self, clips, window_seconds: float, threshold: float):
        """-> (per-clip frame sums, lengths): the locator windowed, its logits the gate of the windowed frames kernel."""
        W = self._window_samples(window_seconds)
        logits = window.windowed_locator(self._need("locator"), clips, W, self.locator_precision)
        fsum = window.windowed_detector_frame_sums(self._need("detector"), clips, logits, localize.gate_threshold(threshold), W,
                                                   self.detector_precision)
        lengths = [int(clips.shape[-1])] * clips.shape[0] if isinstance(clips, torch.Tensor) else [int(c.numel()) for c in clips]
        return fsum, lengths

    @torch.no_grad()
    def detect_clips(self, clips, window_seconds: float = 30.0, localized: bool = False, threshold: float = 0.5):
        """-> (bits [B,16] int32, mean_prob [B,16]) for clips of any lengths, windowed.  localized=True: the masked decode of
        detect_localized_batch instead, -> (bits, prob, coverage [B] float64)."""
        if localized:
            fsum, lengths = self._clip_frame_sums(clips, window_seconds, threshold)
            per_clip = list(fsum) if not isinstance(fsum, torch.Tensor) else [fsum[b] for b in range(fsum.shape[0])]
            probs, counts = [], []
            for f in per_clip:                                  # one [1, nb + 1, Fr_b] tensor per clip: the clips' Fr differ
                p, c = ops.frames_reduce(f.unsqueeze(0), [(0, 0, f.shape[1])])
                probs.append(p)
                counts.append(c)
            prob, count = torch.cat(probs), torch.cat(counts)
            return (prob >= 0.5).to(torch.int32), prob, count / torch.tensor(lengths, dtype=torch.float64, device=count.device)
        mp = window.windowed_detector_mean_prob(self._need("detector"), clips, self._window_samples(window_seconds),
                                                self.detector_precision)
        return (mp >= 0.5).to(torch.int32), mp

    @torch.no_grad()
    def detect_segments_clips(self, clips, window_seconds: float = 30.0, threshold: float = 0.5, min_on: float = 0.5, min_gap_frames: int = 2,
                              min_len_frames: int = 5, split=None) -> List[List[Segment]]:
        """detect_segments_batch for clips of any lengths, windowed."""
        fsum, lengths = self._clip_frame_sums(clips, window_seconds, threshold)
        hop = self._need("detector").hop_length
        if split is not None:
            return self._segments_split(fsum, lengths, hop, min_on, min_gap_frames, min_len_frames, split)
        return self._segments(fsum, lengths, hop, min_on, min_gap_frames, min_len_frames)

    @torch.no_grad()
    def locate_clips(self, clips, window_seconds: float = 30.0):
        """-> sigmoid(locator logits) per clip: a list of [T] tensors, or [B, T] for a [B,1,T] input."""
        out = window.windowed_locator(self._need("locator"), clips, self._window_samples(window_seconds), self.locator_precision)
        if isinstance(out, torch.Tensor):
            return torch.sigmoid(out).squeeze(1)
        return [torch.sigmoid(o) for o in out]

    def open_embed_session(self, watermark_ids, sample_rate: int = 16000, channels: int = 1, strength: float = 1.0):
        """Live watermarking of len(watermark_ids) streams in lockstep.  With the defaults: session.EmbedSession, 16 kHz mono, push(x [S, n]).
        Any other sample_rate, channels or strength: native_session.NativeEmbedSession, push(x [S, C, n]) -> [S, C, k] at the stream's own rate
        and channel count, the arithmetic of embed_native_batch; a rate is refused as embed(native=True) refuses it."""
        if self.snr_floor_db is not None:
            raise ValueError("the lockstep embed sessions have no SNR floor: use open_embed_bank, or set_snr_floor(None)")
        plain = (int(sample_rate), int(channels), float(strength)) == (self.sample_rate, 1, 1.0)
        if not plain and self.channel_snr_floor_db is not None:
            raise ValueError(_NO_LIVE_CHANNEL_FLOOR)
        gen, msg = self._need("generator"), self._messages(watermark_ids)
        if plain:
            return session.EmbedSession(gen, msg, self.generator_precision)
        return native_session.NativeEmbedSession(gen, msg, sample_rate, channels, strength, self.generator_precision)

    def open_detect_session(self, n: int = 1, sample_rate: int = 16000, channels: int = 1):
        """session.DetectSession, or for another rate or channel count native_session.NativeDetectSession (push(x [n, C, k]))."""
        if (int(sample_rate), int(channels)) == (self.sample_rate, 1):
            return session.DetectSession(self._need("detector"), n, self.detector_precision)
        return native_session.NativeDetectSession(self._need("detector"), n, sample_rate, channels, self.detector_precision)

    def open_locate_session(self, n: int = 1, sample_rate: int = 16000, channels: int = 1):
        """session.LocateSession, or for another rate or channel count native_session.NativeLocateSession, whose logits stay on the 16 kHz
        time line."""
        if (int(sample_rate), int(channels)) == (self.sample_rate, 1):
            return session.LocateSession(self._need("locator"), n, self.locator_precision)
        return native_session.NativeLocateSession(self._need("locator"), n, sample_rate, channels, self.locator_precision)

    def open_embed_bank(self, capacity: int = 64, pad_limit: float = 1.5, rates=None, max_channels: int = 2):
        """session.EmbedBank: up to `capacity` live 16 kHz mono streams that open, push and close on their own.
        bank.open(watermark_id) -> slot; bank.push({slot: x [n], ...}) -> {slot: the watermarked samples of the frames that push completed};
        bank.close(slot) -> the rest.  The streams that complete frames on a tick share one generator launch per pad_limit group.
        bank.set_message(slot, watermark_id or None) -> the sample from which the stream carries that id, or (None) no watermark at all:
        the input comes back bit for bit and costs no generator time; bank.open(None) starts that way.
        rates=(48000, 8000, ...): native_bank.NativeEmbedBank, every slot at its own rate and channel count:
        bank.open(watermark_id, sample_rate, channels, strength) with sample_rate one of up to 8 `rates` and channels <= max_channels,
        bank.push({slot: x [C, n]}) -> {slot: [C, k]} at the slot's rate.  A rate is refused as embed(native=True) refuses it.
        With set_snr_floor(db) in force the bank is built under that floor; a later set_snr_floor does not reach it.
        With set_channel_snr_floor(db) in force a bank with `rates` is refused here: open_native_embed_bank builds it under that floor."""
        messages = lambda w: message_to_tensor(self._validate_watermark_id(w).to_bits(), self.watermark_bits)[0]        # noqa: E731
        if rates is None:
            bank = session.EmbedBank(self._need("generator"), capacity, self.generator_precision, pad_limit, messages=messages)
        else:
            if self.channel_snr_floor_db is not None:
                raise ValueError(_NO_LIVE_CHANNEL_FLOOR)
            rates = native_bank.check_rates(rates)                         # before anything is built on the device
            bank = native_bank.NativeEmbedBank(self._need("generator"), rates, capacity, max_channels, self.generator_precision, pad_limit, messages)
        if self.snr_floor_db is not None:
            bank.set_snr_floor(self.snr_floor_db)                          # the bank takes the value at construction
        return bank

    def open_native_embed_bank(self, rates, capacity: int = 64, pad_limit: float = 1.5, max_channels: int = 2, channel_snr_floor_db="instance"):
        """native_bank.NativeEmbedBank as open_embed_bank(rates=...) builds it, under the PER-CHANNEL SNR floor:
        channel_snr_floor_db defaults to the instance's set_channel_snr_floor value ("instance"); a number sets it for this bank, None builds
        the bank without it.  Under the floor a sample leaves only when its whole native frame has its residual (bank.latency_samples(slot) says
        how late), per stream the concatenated output is embed_native_batch's channel floor on the whole recording, a silent channel comes
        back bit for bit, and bank.gains(slot) returns the gains [C, nf] of the frames the slot's last push or close emitted.
        set_snr_floor's value is handed over as open_embed_bank hands it over; with both floors the inner 16 kHz floor carries each slot's
        strength and the channel floor's cap is 1, as for files."""
        db = self.channel_snr_floor_db if isinstance(channel_snr_floor_db, str) and channel_snr_floor_db == "instance" else channel_snr_floor_db
        db = snr_floor.check_db(db)
        rates = native_bank.check_rates(rates)                             # before anything is built on the device
        messages = lambda w: message_to_tensor(self._validate_watermark_id(w).to_bits(), self.watermark_bits)[0]        # noqa: E731
        bank = native_bank.NativeEmbedBank(self._need("generator"), rates, capacity, max_channels, self.generator_precision, pad_limit, messages)
        if self.snr_floor_db is not None:
            bank.set_snr_floor(self.snr_floor_db)
        if db is not None:
            bank.set_channel_snr_floor(db)
        return bank

    def open_detect_bank(self, capacity: int = 64, pad_limit: float = 1.5, rates=None, max_channels: int = 2):
        """session.DetectBank: bank.open() -> slot; bank.push({slot: x [n]}) -> {slot: DetectState over that stream's completed frames}.
        rates=(...): native_bank.NativeDetectBank, bank.open(sample_rate=, channels=), push({slot: x [C, n]})."""
        if rates is None:
            return session.DetectBank(self._need("detector"), capacity, self.detector_precision, pad_limit)
        rates = native_bank.check_rates(rates)
        return native_bank.NativeDetectBank(self._need("detector"), rates, capacity, max_channels, self.detector_precision, pad_limit)

    def open_locate_bank(self, capacity: int = 64, pad_limit: float = 1.5, rates=None, max_channels: int = 2):
        """session.LocateBank: bank.open() -> slot; bank.push({slot: x [n]}) -> {slot: locator logits of the frames that push completed}.
        rates=(...): native_bank.NativeLocateBank, bank.open(sample_rate=, channels=), push({slot: x [C, n]}); the logits stay on the 16 kHz
        time line."""
        if rates is None:
            return session.LocateBank(self._need("locator"), capacity, self.locator_precision, pad_limit)
        rates = native_bank.check_rates(rates)
        return native_bank.NativeLocateBank(self._need("locator"), rates, capacity, max_channels, self.locator_precision, pad_limit)

    def open_segment_session(self, n: int = 1, threshold: float = 0.5, min_on: float = 0.5, min_gap_frames: int = 2, min_len_frames: int = 5,
                             sample_rate: int = 16000, channels: int = 1, capacity: int = 64):
        """Live localized detection of n streams in lockstep, the live twin of detect_segments_batch: session.SegmentSession, push(x [n, k],
        gate=None) returns nothing, poll() -> per stream the Segments that have ended since the last poll, open_segments() the runs still
        open, flush() the rest.  Any other sample_rate or channels: native_session.NativeSegmentSession, push(x [n, C, k]) (no gate there);
        segment times stay seconds on the stream's own clock.  capacity: closed segments the device holds per stream between reads."""
        det, loc = self._need("detector"), self._need("locator")
        kw = dict(threshold=threshold, min_on=min_on, min_gap_frames=min_gap_frames, min_len_frames=min_len_frames,
                  precision=self.detector_precision, locator_precision=self.locator_precision, capacity=capacity)
        if (int(sample_rate), int(channels)) == (self.sample_rate, 1):
            return session.SegmentSession(det, loc, n, sample_rate=self.sample_rate, **kw)
        return native_session.NativeSegmentSession(det, loc, n, sample_rate, channels, **kw)

    def open_segment_bank(self, capacity: int = 64, pad_limit: float = 1.5, threshold: float = 0.5, min_on: float = 0.5, min_gap_frames: int = 2,
                          min_len_frames: int = 5, ring: int = 64, gated: bool = False):
        """session.SegmentBank: live localized detection of up to `capacity` 16 kHz mono streams that open, push and close on their own
        (DESIGN.md section 7d-7).  bank.open() -> slot; bank.push({slot: x [n]}) returns nothing; bank.poll() -> {slot: the Segments that have
        ended since the last poll}; bank.open_segments() -> {slot: the run still open, or None}; bank.close(slot) -> the rest.  gated=True:
        push({slot: (x [n], gate [n])}), the 0 / 1 gate replacing the locator.  ring: closed segments the device holds per slot between reads."""
        return session.SegmentBank(self._need("detector"), self._need("locator"), capacity, pad_limit, threshold, min_on, min_gap_frames,
                                   min_len_frames, ring, gated, self.detector_precision, self.locator_precision, self.sample_rate)

    def open_native_segment_bank(self, rates, max_channels: int = 2, capacity: int = 64, pad_limit: float = 1.5, threshold: float = 0.5,
                                 min_on: float = 0.5, min_gap_frames: int = 2, min_len_frames: int = 5, ring: int = 64, gated: bool = False):
        """native_bank.NativeSegmentBank: open_segment_bank for streams at their own rates (up to 8 `rates`) and channel counts (DESIGN.md section
        7d-8): bank.open(sample_rate=, channels=) -> slot; bank.push({slot: x [C, n]}); poll(), open_segments() and close() as there, segment times
        in seconds on the stream's own clock.  A gate has no native-rate form: gated=True is refused."""
        if gated:
            raise ValueError("a gate is given per 16 kHz sample; a bank at the streams' own rates takes none")
        rates = native_bank.check_rates(rates)
        return native_bank.NativeSegmentBank(self._need("detector"), self._need("locator"), rates, capacity, max_channels, pad_limit=pad_limit,
                                             threshold=threshold, min_on=min_on, min_gap_frames=min_gap_frames, min_len_frames=min_len_frames,
                                             ring=ring, precision=self.detector_precision, locator_precision=self.locator_precision)

    # ------------------------------------------------------------------ reference file API
    def embed(self, audio_path: Union[str, Path], watermark_id: Union[WatermarkID, str, int],
              output_path: Optional[Union[str, Path]] = None, *, native: bool = False, strength: float = 1.0,
              window_seconds: Optional[float] = None) -> Tuple[np.ndarray, int, WatermarkID]:
        """window_seconds (NOT in the reference): run the clip as windows of that length; None = one whole-clip forward.
        native (NOT in the reference): keep the file's own sample rate and channels (embed_native_batch) -> (array [C, Tn], or [Tn] for a
        mono file; the file's sample rate; id), every channel saved at that rate.  strength scales the residual; it needs native."""
        if not native and strength != 1.0:
            raise ValueError("strength other than 1.0 needs native=True (the reference's route adds the residual as it is)")
        try:
            watermark_id = self._validate_watermark_id(watermark_id)
            if native:
                audio, sr = load_audio_native(audio_path)                           # [C, Tn] at the file's rate
                msg = message_to_tensor(watermark_id.to_bits(), self.watermark_bits)
                wm = self.embed_native_batch(audio.unsqueeze(0), sr, msg, strength, window_seconds).squeeze(0)
                if output_path:
                    save_audio(wm, output_path, sr)
                out = wm.cpu().numpy()
                return (out[0] if out.shape[0] == 1 else out), sr, watermark_id
            audio, _ = load_audio(audio_path, self.sample_rate)
            msg = message_to_tensor(watermark_id.to_bits(), self.watermark_bits)
            if window_seconds is None:
                wm = self.embed_batch(audio.unsqueeze(0), msg).squeeze(0)          # [1, T]
            else:
                wm = self.embed_clips(audio.unsqueeze(0), watermark_id, window_seconds).squeeze(0)
            if output_path:
                save_audio(wm, output_path, self.sample_rate)
            return wm.cpu().numpy().squeeze(), self.sample_rate, watermark_id
        except Exception as e:
            logger.error(f"Embedding failed: {str(e)}")
            raise RuntimeError(f"Failed to embed watermark: {str(e)}") from e

    def detect(self, audio_path: Union[str, Path], localized: bool = False, *, window_seconds: Optional[float] = None) -> Tuple[WatermarkID, float]:
        """localized (NOT in the reference): decode only over the samples the locator marks (detect_localized_batch); where it marks
        none, the all-zero id comes back with confidence 0."""
        try:
            audio, _ = load_audio(audio_path, self.sample_rate)
            if localized and window_seconds is None:
                _, mp, _ = self.detect_localized_batch(audio.unsqueeze(0))
            elif localized:
                _, mp, _ = self.detect_clips(audio.unsqueeze(0), window_seconds, localized=True)
            elif window_seconds is None:
                _, mp = self.detect_batch(audio.unsqueeze(0))
            else:
                _, mp = self.detect_clips(audio.unsqueeze(0), window_seconds)
            confidence = mp.mean().item()              # mean of per-bit mean probabilities (core.py:583)
            detected = WatermarkID.custom(tensor_to_message(mp))
            return detected, confidence
        except Exception as e:
            logger.error(f"Detection failed: {str(e)}")
            raise RuntimeError(f"Failed to detect watermark: {str(e)}") from e

    def segments(self, audio_path: Union[str, Path], *, window_seconds: Optional[float] = None, split=None) -> List[Segment]:
        """NOT in the reference: the file's watermarked Segments (start_s, end_s, watermark, confidence, coverage), each decoded over its
        own marked samples; an empty list where the locator marks nothing.  split: a localize.SplitRule, as detect_segments_batch takes."""
        try:
            audio, _ = load_audio(audio_path, self.sample_rate)
            if window_seconds is None:
                return self.detect_segments_batch(audio.unsqueeze(0), split=split)[0]
            return self.detect_segments_clips(audio.unsqueeze(0), window_seconds, split=split)[0]
        except Exception as e:
            logger.error(f"Segment detection failed: {str(e)}")
            raise RuntimeError(f"Failed to detect watermark segments: {str(e)}") from e

    def locate(self, audio_path: Union[str, Path], *, window_seconds: Optional[float] = None) -> np.ndarray:
        try:
            audio, _ = load_audio(audio_path, self.sample_rate)
            if window_seconds is None:
                mask = self.locate_batch(audio.unsqueeze(0)).squeeze()
            else:
                mask = self.locate_clips(audio.unsqueeze(0), window_seconds).squeeze()
            n = audio.shape[-1]
            if mask.dim() == 1 and mask.shape[0] != n:          # core.py:638-644 (never hit: same length)
                mask = torch.nn.functional.interpolate(mask[None, None], size=n, mode="linear",
                                                       align_corners=False).squeeze()
            return mask.cpu().numpy()
        except Exception as e:
            logger.error(f"Localization failed: {str(e)}")
            raise RuntimeError(f"Failed to locate watermark: {str(e)}") from e

    def verify(self, audio_path: Union[str, Path],
               expected_watermark: Union[WatermarkID, str, int], localized: bool = False) -> bool:
        try:
            expected = self._validate_watermark_id(expected_watermark)
            detected, _ = self.detect(audio_path, localized)
            return detected == expected
        except Exception as e:
            logger.error(f"Verification failed: {str(e)}")
            raise RuntimeError(f"Failed to verify watermark: {str(e)}") from e

    def _validate_watermark_id(self, watermark_id) -> WatermarkID:
        if not isinstance(watermark_id, WatermarkID):
            try:
                watermark_id = WatermarkID.custom(watermark_id)
            except (ValueError, TypeError) as e:
                raise ValueError(
                    f"Invalid watermark_id: {e}. Use WatermarkID.for_creator(), .for_timestamp(), etc. "
                    f"or provide a 16-bit binary string, int (0-65535), or 2 bytes.")
        return watermark_id
