"""Whole-video grounding: frames in, one box per frame out — every frame through the backbone ONCE.

The reference grounds a video one window at a time (test_DCNet.py re-runs the n_frame model per window; ``getChunk``,
dataset/vid_loader.py:143-180, builds the windows), so a frame is encoded once per window it appears in and the affinity of two
frames is computed once in each of their windows.  Here:

  * every frame goes through Darknet-53, ``mapping_visu`` and the normalisation once, into a per-scale FEATURE BANK (fp32 rows and
    their f16 two-piece split form, ``dcn_bank_write``);
  * the co-attention of two frames is computed once: one affinity yields what each of the two takes from the other
    (``dcn_coattn_bank_fwd`` reads bank rows through strides: the pairs of distance d are bank[a0:a0+n] against bank[a0+d:a0+d+n]);
  * the language branch runs once per query; nothing before ``sim_score`` and the fusion head depends on the sentence, so any
    number of queries share the visual work;
  * the temporal re-scoring reads the candidates of the centres in place (``dcn_post_fusion_bank``);
  * optionally (``link=TubeLink()``) the candidates of ALL centres are joined into one track per query: an NMS mask per centre and a
    Viterbi path over IoU + correspondence-feature transitions (``csrc/tube.hip``);
  * for streams, ``FuseStream`` / ``TubeStream`` (``vg.tube_stream(lag)``) do the last two while the frames arrive: they take the parts
    of ``push`` one by one, keep a constant amount of state and hand a centre's fused choice and tube entry out a fixed number of
    centres later.

The window rule is the reference's (``getChunk``):

    window of centre i  =  frames i - K//2 ... i + ceil(K/2) - 1,   centre slot K//2

    vg = VideoGrounder(model, n_frame=5, border="valid", chunk=32, topk=None)
    res = vg.run(image, word_id, meta=None)            # image (F,3,S,S) CUDA, word_id (Q,L) or (L,)
    # or incrementally, for streams and long videos:
    vg.reset(word_id); out = vg.push(image_chunk); ...; out = vg.flush()

Precision modes (``ops.set_precision``; latched at ``reset``): "fp32" as above, and "bf16s" (bf16 storage), where the bank of a scale
holds the rows in bf16 (the centre half of ``corr_conv``'s bf16 input) plus ONE fp32-sized operand of the co-attention — the split
form where its products run on gemm3.hip, the fp32 rows where they do not (``dcn_bank_write_b16``, ``dcn_coattn_bank_form``): 6 bytes
per value instead of 8.  The attended features land in a dense fp32 scratch and ``dcn_bank_concat_b16`` writes the bf16 concat that
``corr_conv`` reads as it is.  The rounding points are those of the windowed model on bf16 storage: ``mapping_visu`` hands out fp32,
normalised in fp32; the co-attention reads the f16 high piece of 8192 f; the concat is rounded to bf16 once.

``python -m dcnet_amd.video --synthetic --frames 64 --n-frame 5 [--precision bf16s]`` runs it on synthetic frames and prints frames/s.
"""
from __future__ import annotations

import math
import os
from dataclasses import dataclass, field
from typing import List, Optional, Sequence, Tuple

import torch

BORDERS = ("valid", "replicate")
BANK_BYTES_PER_VALUE = {"fp32": 4 + 4, "bf16s": 2 + 4}      # precision modes that have the path: fp32 rows + split | bf16 rows + one of the two


# ---- host logic (pure Python) -------------------------------------------------------------------------------------------------
def _check_window(n_frame) -> int:
    if not isinstance(n_frame, int) or isinstance(n_frame, bool) or n_frame < 2:
        raise ValueError(f"n_frame = {n_frame!r}: a window needs at least 2 frames (an int >= 2)")
    return n_frame


def _check_border(border) -> str:
    if border not in BORDERS:
        raise ValueError(f"border = {border!r}: expected one of {BORDERS}")
    return border


def window_offsets(n_frame: int) -> List[int]:
    """Frame offsets of a window relative to its centre, in window order (the centre, offset 0, sits in slot n_frame // 2)."""
    K = _check_window(n_frame)
    return list(range(-(K // 2), (K + 1) // 2))


def centres(frames: int, n_frame: int, border: str = "valid") -> List[int]:
    """The frames that get an answer.  "valid": every centre whose window lies inside the video; "replicate": every frame, window
    indices clamped to [0, frames - 1] (the ``numpy.clip`` that ``getChunk`` carries)."""
    K = _check_window(n_frame)
    if _check_border(border) == "replicate":
        return list(range(frames))
    return list(range(K // 2, frames - (K + 1) // 2 + 1))


def reference_centres(frames: int, n_frame: int) -> List[int]:
    """The centres ``getChunk`` produces: the "valid" ones without the last (it drops a centre i with i + ceil(K/2) > frames - 1,
    although that window still fits) — for people who reproduce the reference's numbers."""
    K = _check_window(n_frame)
    return list(range(K // 2, frames - (K + 1) // 2))


def window_frames(centre: int, frames: int, n_frame: int, border: str = "valid") -> List[int]:
    """Frame indices of the window of ``centre``, in window order (clamped under "replicate")."""
    w = [centre + o for o in window_offsets(n_frame)]
    if _check_border(border) == "replicate":
        return [min(max(j, 0), frames - 1) for j in w]
    if w[0] < 0 or w[-1] > frames - 1:
        raise ValueError(f"frame {centre} is no \"valid\" centre of a video of {frames} frames with n_frame = {n_frame}")
    return w


def _multiplicity(i: int, j: int, K: int, border: str, total: Optional[int]) -> int:
    """How many slots of centre i's window (the centre slot excluded) hold frame j; 0 if i is no centre.  ``total`` None: the
    length of the video is not known yet (nothing clamps from above, no centre is excluded from above)."""
    lo, hi = -(K // 2), (K + 1) // 2 - 1
    if border == "valid":
        if i < K // 2 or (total is not None and i > total - (K + 1) // 2):
            return 0
        return int(j != i and lo <= j - i <= hi)
    top = math.inf if total is None else total - 1
    return sum(1 for o in range(lo, hi + 1) if o != 0 and min(max(i + o, 0), top) == j)


@dataclass
class PairPlan:
    """Batched co-attention work.  ``runs``: (d, a0, n, fwd, bwd) — the n frame pairs (a, a + d), a = a0 ... a0 + n - 1, of
    distance d > 0; fwd: centre a takes from frame a + d (+d is a window offset), bwd: centre a + d takes from frame a (-d is one).
    ``border``: (a, b, w_ab, w_ba), a <= b — single pairs whose results count w_ab times for centre a and w_ba times for centre b
    (clamped windows; a == b is a self pair, w_ba = 0).  Every attended feature enters its centre's mean with weight
    multiplicity / (n_frame - 1)."""
    runs: List[Tuple[int, int, int, bool, bool]] = field(default_factory=list)
    border: List[Tuple[int, int, int, int]] = field(default_factory=list)

    def contributions(self) -> List[Tuple[int, int, int]]:
        """(centre, neighbour frame, multiplicity) of everything the plan computes."""
        out = []
        for d, a0, n, fwd, bwd in self.runs:
            for a in range(a0, a0 + n):
                if fwd:
                    out.append((a, a + d, 1))
                if bwd:
                    out.append((a + d, a, 1))
        for a, b, w_ab, w_ba in self.border:
            if w_ab:
                out.append((a, b, w_ab))
            if w_ba:
                out.append((b, a, w_ba))
        return out

    def affinities(self) -> List[Tuple[int, int]]:
        """The frame pairs (a, b), a <= b, whose affinity matrix the plan computes (one entry per computation)."""
        return [(a, a + d) for d, a0, n, _, _ in self.runs for a in range(a0, a0 + n)] + [(a, b) for a, b, _, _ in self.border]


def pair_plan(first: int, last: int, n_frame: int, border: str = "valid", total: Optional[int] = None) -> PairPlan:
    """The work that becomes possible when frames ``first`` ... ``last - 1`` have been encoded (all earlier frames are in the bank):
    every pair whose LATER frame is one of them, so that no affinity is computed twice however the video is cut into chunks.
    ``total``: frames of the whole video if known (``run``); None while streaming — then, under "valid", centres near the end get
    contributions before it is known whether their window fits (dropped at ``flush`` if not), and under "replicate" the clamp at
    the last frame is made up for by ``flush_plan``."""
    K = _check_window(n_frame); _check_border(border)
    plan = PairPlan()
    for d in range(1, K // 2 + 1):
        run = None                                     # [a0, n, fwd, bwd]
        for b in range(max(first, d), last):
            a = b - d
            w_ab, w_ba = _multiplicity(a, b, K, border, total), _multiplicity(b, a, K, border, total)
            if w_ab > 1 or w_ba > 1:
                plan.border.append((a, b, w_ab, w_ba))
                flags = None
            else:
                flags = (bool(w_ab), bool(w_ba)) if (w_ab or w_ba) else None
            if run is not None and (flags is None or flags != (run[2], run[3])):
                plan.runs.append((d, run[0], run[1], run[2], run[3])); run = None
            if flags is not None:
                if run is None:
                    run = [a, 0, flags[0], flags[1]]
                run[1] += 1
        if run is not None:
            plan.runs.append((d, run[0], run[1], run[2], run[3]))
    for b in range(first, last):
        w = _multiplicity(b, b, K, border, total)
        if w:
            plan.border.append((b, b, w, 0))
    return plan


def flush_plan(frames: int, n_frame: int, border: str = "valid") -> PairPlan:
    """What a stream of unknown length still owes once it ends after ``frames`` frames: under "replicate", the window slots of the
    last centres that clamp to the last frame (these few affinities are computed a second time: a stream does not know its last
    frame when it sees it).  Empty under "valid"."""
    K = _check_window(n_frame); _check_border(border)
    plan = PairPlan()
    if border == "replicate" and frames > 0:
        j = frames - 1
        for i in range(max(0, frames - (K + 1) // 2), frames):
            extra = _multiplicity(i, j, K, border, frames) - _multiplicity(i, j, K, border, None)
            if extra:
                plan.border.append((i, j, extra, 0))
    return plan


# ---- results ------------------------------------------------------------------------------------------------------------------
@dataclass
class VideoResult:
    """Device tensors; n = number of centres, Q = number of queries.  ``outbox[q][s]``, ``sim[q][s]``, ``loc[q][s]``,
    ``only_obj[q][s]``: the n_frame model's outputs of query q on scale s with the centres as the batch dimension; ``corr_feat[s]``
    (n,E,g,g) is shared by the queries.  ``boxes`` (Q,n,4): ``losses.decode_boxes`` (letterbox pixels), or source pixels when the
    letterbox meta was given.  With ``topk``: ``cand_boxes`` (Q,n,k,4), ``cand_scores`` (Q,n,k), ``cand_feats`` (Q,n,k,E) and the
    temporally fused choice ``best`` (Q,n), ``fused`` (Q,n,k), ``fused_boxes`` (Q,n,4).  With ``link``: ``cand_keep`` (Q,n,k) bool, the
    candidates that survive the NMS, and the linked track ``tube`` (Q,n) int64 (candidate index per centre), ``tube_score`` (Q,),
    ``tube_boxes`` (Q,n,4)."""
    centres: torch.Tensor
    outbox: List[List[torch.Tensor]]
    sim: List[List[torch.Tensor]]
    loc: List[List[torch.Tensor]]
    corr_feat: List[torch.Tensor]
    only_obj: List[List[torch.Tensor]]
    boxes: torch.Tensor
    cand_boxes: Optional[torch.Tensor] = None
    cand_scores: Optional[torch.Tensor] = None
    cand_feats: Optional[torch.Tensor] = None
    best: Optional[torch.Tensor] = None
    fused: Optional[torch.Tensor] = None
    fused_boxes: Optional[torch.Tensor] = None
    cand_keep: Optional[torch.Tensor] = None
    tube: Optional[torch.Tensor] = None
    tube_score: Optional[torch.Tensor] = None
    tube_boxes: Optional[torch.Tensor] = None

    def query(self, q: int = 0):
        """The n_frame model's return tuple (outbox, sim, loc, corr_feat, only_obj) of query q."""
        return self.outbox[q], self.sim[q], self.loc[q], self.corr_feat, self.only_obj[q]

    @staticmethod
    def cat(parts: Sequence["VideoResult"]) -> "VideoResult":
        parts = [p for p in parts if p is not None]
        if not parts:
            raise ValueError("VideoResult.cat: no centres (the video is shorter than a window?)")
        if len(parts) == 1:
            return parts[0]
        Q = len(parts[0].outbox)
        per_q = lambda name: [[torch.cat([getattr(p, name)[q][s] for p in parts]) for s in range(3)] for q in range(Q)]
        opt = lambda name: None if getattr(parts[0], name) is None else torch.cat([getattr(p, name) for p in parts], dim=1)
        return VideoResult(centres=torch.cat([p.centres for p in parts]), outbox=per_q("outbox"), sim=per_q("sim"), loc=per_q("loc"),
                           corr_feat=[torch.cat([p.corr_feat[s] for p in parts]) for s in range(3)], only_obj=per_q("only_obj"),
                           boxes=torch.cat([p.boxes for p in parts], dim=1), cand_boxes=opt("cand_boxes"),
                           cand_scores=opt("cand_scores"), cand_feats=opt("cand_feats"), cand_keep=opt("cand_keep"))


@dataclass
class TubeLink:
    """How ``VideoGrounder.link`` joins the candidates of consecutive centres into one track per query (``postprocess.link_tubes``).
    iou_weight, feat_weight  weights (>= 0) of the IoU and of the correspondence-feature dot product of two consecutive candidates
    nms_iou   IoU threshold of the greedy NMS among a centre's candidates (``postprocess.nms_keep``); None: no NMS
    unary     "score": the candidates' confidences; "fused": their temporally fused scores (``fuse``)"""
    iou_weight: float = 1.0
    feat_weight: float = 1.0
    nms_iou: Optional[float] = 0.6
    unary: str = "score"

    def __post_init__(self):
        if self.unary not in ("score", "fused"):
            raise ValueError(f"TubeLink.unary = {self.unary!r}: expected \"score\" or \"fused\"")
        if not (self.iou_weight >= 0 and self.feat_weight >= 0):
            raise ValueError(f"TubeLink: weights must be >= 0 (iou_weight = {self.iou_weight!r}, feat_weight = {self.feat_weight!r})")
        if self.nms_iou is not None and not 0 <= self.nms_iou <= 1:
            raise ValueError(f"TubeLink.nms_iou = {self.nms_iou!r}: an IoU threshold in [0, 1], or None for no NMS")


class VideoGrounder:
    """Grounds every frame of a video against one or more sentences (module docstring).

    model    a ``dcnet_amd.model.grounding_model`` (``model.DCNet_model`` and ``model.test_DCNet_model`` hand out the same class)
             in eval mode.  Precision: "fp32" (the feature bank holds fp32 rows and their f16 two-piece split) or "bf16s" (bf16
             rows and one of the two, module docstring), whichever is set at ``reset``; any other mode of ``ops.set_precision``
             raises a RuntimeError that names it, and so does a ``push`` / ``flush`` under another mode than its ``reset``.
    n_frame  K, frames per window (>= 2); border "valid" | "replicate" (``centres``)
    chunk    frames encoded per step: bounds the memory of the bank rows, concat buffers and the affinity workspace (the
             co-attention sub-batches by ``ops.COATTN_BANK_WS_BYTES`` on its own)
    topk     k: also the k best candidates of every centre and their temporal fusion over windows of n_frame centres
             (n_frame <= 32, k <= 64)
    link     a ``TubeLink``: also one temporally consistent track per query through the candidates of all centres (needs ``topk``);
             None: nothing is linked and the tube fields of the result stay None

    ``push`` keeps the bank rows of the last n_frame // 2 frames (no pair reaches further back; per scale, both tensors of the mode) and the
    unfinished means of the last ceil(n_frame / 2) - 1 centres between calls, so chunked and streamed runs encode every frame once
    too.  Nothing here synchronises the host with the device."""

    def __init__(self, model, n_frame: int = 5, border: str = "valid", chunk: int = 32, topk: Optional[int] = None,
                 link: Optional[TubeLink] = None):
        from .model import grounding_model
        self.n_frame, self.border = _check_window(n_frame), _check_border(border)
        if not isinstance(model, grounding_model):
            raise TypeError(f"model: expected a dcnet_amd.model.grounding_model, got {type(model).__name__}")
        if model.training:
            raise ValueError("model is in train mode: VideoGrounder is the inference path, call model.eval() first")
        if not isinstance(chunk, int) or chunk < 1:
            raise ValueError(f"chunk = {chunk!r}: frames per step, an int >= 1")
        if topk is not None and (not isinstance(topk, int) or not 1 <= topk <= 64 or n_frame > 32):
            raise ValueError(f"topk = {topk!r} with n_frame = {n_frame}: the temporal fusion takes topk in 1 ... 64 and n_frame <= 32")
        if link is not None and not isinstance(link, TubeLink):
            raise TypeError(f"link: expected a dcnet_amd.video.TubeLink or None, got {type(link).__name__}")
        if link is not None and topk is None:
            raise ValueError("link: tube linking joins the top-k candidates of the centres, give topk as well")
        self.model, self.chunk, self.topk, self._link = model, chunk, topk, link
        self._lang = None

    # ---- state ----------------------------------------------------------------------------------------------------------------
    def reset(self, word_id: torch.Tensor, total: Optional[int] = None) -> None:
        """Start a video: run the language branch, once, for the (Q,L) or (L,) token ids.  ``total``: frames of the whole video if
        known in advance."""
        from . import ops
        m = self.model
        if m.training:
            raise ValueError("model is in train mode: VideoGrounder is the inference path, call model.eval() first")
        if not (isinstance(word_id, torch.Tensor) and word_id.is_cuda):
            raise ValueError("word_id: expected a CUDA tensor of token ids (Q,L) or (L,) (HIP kernels only, no CPU path)")
        if ops.get_precision() not in BANK_BYTES_PER_VALUE:
            raise RuntimeError(f"VideoGrounder runs in the \"fp32\" and \"bf16s\" precision modes (the two that have the feature-bank "
                               f"path); the current mode is {ops.get_precision()!r}")
        self._mode = ops.get_precision()                          # latched: the banks of a video are in ONE mode's layout
        if word_id.dim() == 1:
            word_id = word_id.unsqueeze(0)
        dev = word_id.device
        main = torch.cuda.current_stream()
        with torch.no_grad():
            if ops.use_amax():
                ops.amax_begin_step(dev)
            side = m._side_stream(dev) if m.language_stream else main
            side.wait_stream(main)
            with torch.cuda.stream(side):
                wid, flang, context, embedded = m._language(word_id)
                flang_attn, flang_loc = m._phrases(context, embedded, wid)
        self._lang = {"side": side, "joined": side is main, "flang": flang, "attn": flang_attn, "loc": flang_loc, "Q": word_id.shape[0]}
        K = self.n_frame
        self._total, self._seen = total, 0
        self._bank = None                                         # per scale (bank, split) of frames [_seen - keep, _seen); "bf16s":
        self._form = None                                         # (rows16, split if _form[s] else bank), _form[s] = coattn_bank_form
        self._acc = None                                          # per scale: unfinished means of centres [_acc_lo, ...)
        self._acc_lo = K // 2 if self.border == "valid" else 0    # first centre not handed out yet
        self._meta = []                                           # device (ratio, dw, dh, frame_hw) of frames [_meta_lo, ...)
        self._meta_lo, self._meta_all = 0, False                  # _meta_all: run() uploaded the whole video's meta up front

    def _join_language(self):
        st = self._lang
        if not st["joined"]:
            main = torch.cuda.current_stream()
            main.wait_stream(st["side"])
            for t_ in (st["flang"], st["attn"], st["loc"]):
                t_.record_stream(main)
            st["joined"] = True

    def _check_mode(self, where: str) -> None:
        from . import ops
        if ops.get_precision() != self._mode:
            raise RuntimeError(f"VideoGrounder.{where}: the precision mode is {ops.get_precision()!r} but this video was reset under "
                               f"{self._mode!r}; its banks are in that mode's layout (reset again, or set the mode back)")

    def bank_bytes_per_frame(self, size: Optional[int] = None) -> int:
        """Bytes of feature bank the grounder keeps per frame, all three scales: (size/32 * 2^s)^2 pixels of emb_size values, 8 bytes
        per value in "fp32" (fp32 rows + split), 6 in "bf16s" (bf16 rows + split OR fp32 rows).  The mode is the latched one while a
        video is open, else the current one; ``size`` defaults to the frame size of the last ``push``."""
        from . import ops
        mode = self._mode if self._lang is not None else ops.get_precision()
        if mode not in BANK_BYTES_PER_VALUE:
            raise RuntimeError(f"bank_bytes_per_frame: no feature-bank path in the precision mode {mode!r} (\"fp32\" and \"bf16s\" have it)")
        if size is None:
            size = getattr(self, "_size", None)
            if size is None:
                raise ValueError("bank_bytes_per_frame: size not given and no frame pushed yet")
        return sum((size // 32 * 2 ** s) ** 2 for s in range(3)) * self.model.emb_size * BANK_BYTES_PER_VALUE[mode]

    # ---- one step -------------------------------------------------------------------------------------------------------------
    def _contribute(self, s, bank, split, base, acc, h, w, plan: PairPlan):
        from . import ops
        m, K = self.model, self.n_frame
        hw, e = bank.shape[1], bank.shape[2]
        lo = self._acc_lo

        def one_b16(a, d, n, fwd, bwd, w_f, w_b):
            # bank = the bf16 rows, split = the one operand form the co-attention of this scale reads (_form[s])
            attn = torch.empty(((int(fwd) + int(bwd)) * n, hw, e), dtype=torch.float32, device=bank.device)
            af = attn[:n] if fwd else None
            ab = attn[n if fwd else 0:] if bwd else None
            on3 = self._form[s]
            ops.coattn_bank_fwd(None if on3 else split, split if on3 else None, a - base, d, n, af, ab, m.temperature)
            if fwd:
                cat = ops.bank_concat_b16(bank, a - base, af)
                m._corr_accumulate(s, cat.view(n, h, w, 2 * e), acc[a - lo:a - lo + n].view(n, h, w, e), w_f / (K - 1))
            if bwd:
                cat = ops.bank_concat_b16(bank, a + d - base, ab)
                m._corr_accumulate(s, cat.view(n, h, w, 2 * e), acc[a + d - lo:a + d - lo + n].view(n, h, w, e), w_b / (K - 1))

        def one(a, d, n, fwd, bwd, w_f, w_b):
            if self._mode == "bf16s":
                return one_b16(a, d, n, fwd, bwd, w_f, w_b)
            cat = torch.empty(((int(fwd) + int(bwd)) * n, hw, 2 * e), dtype=torch.float32, device=bank.device)
            cf = cat[:n] if fwd else None
            cb = cat[n if fwd else 0:] if bwd else None
            if fwd:
                cf[..., :e].copy_(bank[a - base:a - base + n])
            if bwd:
                cb[..., :e].copy_(bank[a + d - base:a + d - base + n])
            ops.coattn_bank_fwd(bank, split, a - base, d, n, None if cf is None else cf[..., e:], None if cb is None else cb[..., e:],
                                m.temperature)
            if fwd:
                m._corr_accumulate(s, cf.view(n, h, w, 2 * e), acc[a - lo:a - lo + n].view(n, h, w, e), w_f / (K - 1))
            if bwd:
                m._corr_accumulate(s, cb.view(n, h, w, 2 * e), acc[a + d - lo:a + d - lo + n].view(n, h, w, e), w_b / (K - 1))

        for d, a0, n, fwd, bwd in plan.runs:
            one(a0, d, n, fwd, bwd, 1.0, 1.0)
        for a, b, w_ab, w_ba in plan.border:
            one(a, b - a, 1, bool(w_ab), bool(w_ba), float(w_ab), float(w_ba))

    def _emit(self, hi: int, size: int) -> Optional[VideoResult]:
        """Heads of the finished centres [_acc_lo, hi) for every query."""
        from . import losses, postprocess
        m, lo = self.model, self._acc_lo
        nc = hi - lo
        if nc <= 0:
            return None
        self._join_language()
        st = self._lang
        corr = []
        for s in range(3):
            gh, gw = self._grid_hw[s]
            done = self._acc[s][:nc]
            self._acc[s] = self._acc[s][nc:].clone()
            corr.append(done.view(nc, gh, gw, done.shape[-1]))
        corr_nchw = [c.permute(0, 3, 1, 2) for c in corr]
        dev = corr[0].device
        outs, sims, locs, onlys, boxes, cands = [], [], [], [], [], []
        meta = None
        if self._meta:
            i0 = lo - self._meta_lo
            meta = [torch.cat([mm[k] for mm in self._meta])[i0:i0 + nc] for k in range(4)]
        elif self.topk is not None:
            meta = [torch.ones(nc, device=dev), torch.zeros(nc, device=dev), torch.zeros(nc, device=dev),
                    torch.full((nc, 2), size, dtype=torch.int64, device=dev)]
        for q in range(st["Q"]):
            ex = lambda t: t[q:q + 1].expand(nc, *t.shape[1:]).contiguous()
            flang, fattn, floc = ex(st["flang"]), ex(st["attn"]), ex(st["loc"])
            res = [m._score_scale(s, corr[s], flang, fattn) for s in range(3)]
            sim = [r[0] for r in res]
            outbox, loc, only_obj = m._head(sim, [r[1] for r in res], floc)
            outs.append(list(outbox)); sims.append(sim); locs.append(list(loc)); onlys.append(list(only_obj))
            if self._meta:
                b1 = postprocess.topk_candidates(outbox, corr_nchw, size, 1, *meta)[0][:, 0]
            else:
                b1 = losses.decode_boxes(outbox, size)
            boxes.append(b1)
            if self.topk is not None:
                cands.append(postprocess.topk_candidates(outbox, corr_nchw, size, self.topk, *meta)[:3])
        res = VideoResult(centres=torch.arange(lo, hi, device=dev), outbox=outs, sim=sims, loc=locs, corr_feat=corr_nchw, only_obj=onlys,
                          boxes=torch.stack(boxes))
        if cands:
            res.cand_boxes, res.cand_scores, res.cand_feats = (torch.stack([c[k] for c in cands]) for k in range(3))
            if self._link is not None:
                Q, k = res.cand_scores.shape[0], res.cand_scores.shape[2]
                if self._link.nms_iou is None:
                    res.cand_keep = torch.ones((Q, nc, k), dtype=torch.bool, device=dev)
                else:
                    res.cand_keep = postprocess.nms_keep(res.cand_boxes.view(Q * nc, k, 4), self._link.nms_iou).view(Q, nc, k)
        self._acc_lo = hi
        return res

    def _upload_meta(self, meta, n: int, size: int, dev):
        from .postprocess import letterbox_frame
        ratio, dw, dh = ([float(v) for v in x] for x in meta)
        if not (len(ratio) == len(dw) == len(dh) == n):
            raise ValueError(f"meta: (ratio, dw, dh) must have one entry per frame ({n})")
        hw = [letterbox_frame(size, r, a, b) for r, a, b in zip(ratio, dw, dh)]
        up = lambda v, dt: torch.tensor(v, dtype=dt).pin_memory().to(dev, non_blocking=True)      # (page-locked: a true async copy)
        self._meta.append((up(ratio, torch.float32), up(dw, torch.float32), up(dh, torch.float32), up(hw, torch.int64).reshape(n, 2)))

    @torch.no_grad()
    def push(self, image: torch.Tensor, meta=None) -> Optional[VideoResult]:
        """The next frames of the video, (n,3,S,S) CUDA fp32 (any n >= 1; more than ``chunk`` frames are taken in steps).  ``meta``:
        (ratio, dw, dh) per frame of this call (what ``prep.Prepared`` carries), for boxes in source pixels — for every call of a
        video or for none.  Returns the results of the centres that were completed, or None."""
        from . import ops
        if self._lang is None:
            raise RuntimeError("VideoGrounder.push: call reset(word_id) first")
        if not (isinstance(image, torch.Tensor) and image.is_cuda and image.dim() == 4 and image.shape[0] >= 1):
            raise ValueError("image: expected a CUDA tensor (n,3,S,S) (HIP kernels only, no CPU path)")
        self._check_mode("push")
        if image.shape[0] > self.chunk:
            parts = []
            for i0 in range(0, image.shape[0], self.chunk):
                mm = None if meta is None else tuple(x[i0:i0 + self.chunk] for x in meta)
                parts.append(self.push(image[i0:i0 + self.chunk], mm))
            return VideoResult.cat(parts) if any(p is not None for p in parts) else None
        m, K, dev = self.model, self.n_frame, image.device
        n_new, size = image.shape[0], image.shape[-1]
        if meta is not None:
            if self._seen and not self._meta:
                raise ValueError("meta: given for this call but not for the earlier frames of the video")
            self._upload_meta(meta, n_new, size, dev)            # (before the step's kernels are queued)
        elif self._meta and not self._meta_all:
            raise ValueError("meta: given for the earlier frames of the video but not for this call")
        p0, p1 = self._seen, self._seen + n_new
        keep = 0 if self._bank is None else self._bank[0][0].shape[0]
        base = p0 - keep
        if ops.use_amax():
            ops.amax_begin_step(dev)
        raw = m.visumodel.forward_nhwc(image.float(), taps_b16=True)
        m._head_filter_banks()
        plan = pair_plan(p0, p1, K, self.border, self._total)
        n_acc = max(0, p1 - self._acc_lo)
        banks, accs = [], []
        b16 = self._mode == "bf16s"
        if b16 and self._form is None:
            self._form = [None] * 3
        for s in range(3):
            x = m._map_scale(s, raw[s])                           # (fp32 in either mode: the bank normalises in fp32)
            _, h, w, e = x.shape
            bank = torch.empty((keep + n_new, h * w, e), dtype=torch.bfloat16 if b16 else torch.float32, device=dev)
            split = torch.empty((keep + n_new, h * w, e), dtype=torch.float32, device=dev)
            if keep:
                bank[:keep].copy_(self._bank[s][0]); split[:keep].copy_(self._bank[s][1])
            if b16:
                if m.corr_conv[s][0].__dict__.get("_dcn_bank") is None:
                    raise RuntimeError("VideoGrounder, \"bf16s\": corr_conv reads the bf16 concat through its prepared filter bank "
                                       "(ops.FILTER_BANKS is off)")
                form = ops.coattn_bank_form(h * w, e)
                if self._form[s] is not None and self._form[s] != form:
                    raise RuntimeError(f"VideoGrounder.push: the co-attention form of scale {s} changed within a video (a tuning knob?)")
                self._form[s] = form
                ops.bank_write_b16(x, bank[keep:], bank=None if form else split[keep:], split=split[keep:] if form else None)
            else:
                ops.bank_write(x, bank[keep:], split[keep:])
            acc = torch.zeros((n_acc, h * w, e), dtype=torch.float32, device=dev)
            if self._acc is not None and self._acc[s].shape[0]:
                acc[:self._acc[s].shape[0]].copy_(self._acc[s])
            self._contribute(s, bank, split, base, acc, h, w, plan)
            banks.append((bank, split)); accs.append(acc)
        self._acc = accs
        k2 = min(K // 2, keep + n_new)
        self._bank = [(b[b.shape[0] - k2:].clone(), sp[sp.shape[0] - k2:].clone()) if k2 < b.shape[0] else (b, sp) for b, sp in banks]
        self._seen, self._size = p1, size
        self._grid_hw = [(int(round(math.sqrt(b.shape[1]))),) * 2 for b, _ in banks]
        return self._emit(p1 - (K + 1) // 2 + 1, size)

    @torch.no_grad()
    def flush(self) -> Optional[VideoResult]:
        """End of the video: the centres that were waiting for it (border "replicate"); under "valid" the unfinished ones are
        dropped.  Returns their results, or None; the grounder needs a ``reset`` before the next video."""
        if self._lang is None:
            raise RuntimeError("VideoGrounder.flush: call reset(word_id) first")
        self._check_mode("flush")
        out = None
        if self.border == "replicate" and self._seen > self._acc_lo:
            if self._total is None:
                plan = flush_plan(self._seen, self.n_frame, self.border)
                base = self._seen - self._bank[0][0].shape[0]
                for s in range(3):
                    h, w = self._grid_hw[s]
                    self._contribute(s, self._bank[s][0], self._bank[s][1], base, self._acc[s], h, w, plan)
            out = self._emit(self._seen, self._size)
        self._lang = None
        self._bank = self._acc = None
        return out

    def fuse(self, res: VideoResult) -> VideoResult:
        """Temporal fusion over the candidates of ALL centres of a video (``topk`` set): window b = the candidates of centres
        b - K//2 ... b - K//2 + K - 1, centres outside the run missing.  Fills best / fused / fused_boxes."""
        from . import ops
        if res.cand_feats is None:
            raise ValueError("fuse: the grounder was built without topk")
        best, fused = zip(*[ops.post_fusion_bank(res.cand_feats[q].contiguous(), res.cand_scores[q].contiguous(), self.n_frame)
                            for q in range(res.cand_feats.shape[0])])
        res.best, res.fused = torch.stack(best), torch.stack(fused)
        res.fused_boxes = torch.gather(res.cand_boxes, 2, res.best[:, :, None, None].expand(-1, -1, 1, 4))[:, :, 0]
        return res

    def link(self, res: VideoResult) -> VideoResult:
        """The linked track of every query through the candidates of ``res`` (``link`` set): ``res`` covers consecutive centres — the
        result of ``run``, or the ``VideoResult.cat`` of the parts of a stream.  Fills tube / tube_score / tube_boxes.  With
        ``TubeLink.unary == "fused"`` the result must have been through ``fuse``."""
        from . import postprocess
        cfg = self._link
        if cfg is None:
            raise ValueError("link: the grounder was built without link")
        if res.cand_keep is None:
            raise ValueError("link: the result carries no candidates of a grounder with link (cand_keep is None)")
        unary = res.cand_scores if cfg.unary == "score" else res.fused
        if unary is None:
            raise ValueError("link: TubeLink.unary is \"fused\" but the result has no fused scores, call fuse(res) first")
        feats = res.cand_feats if cfg.feat_weight > 0 else None
        res.tube, res.tube_score, res.tube_boxes = postprocess.link_tubes(res.cand_boxes, unary, feats, res.cand_keep, cfg.iou_weight,
                                                                          cfg.feat_weight)
        return res

    @torch.no_grad()
    def run(self, image: torch.Tensor, word_id: torch.Tensor, meta=None) -> VideoResult:
        """A whole video at once: image (F,3,S,S) CUDA, word_id (Q,L) or (L,), meta = (ratio, dw, dh) per frame or None."""
        if not (isinstance(image, torch.Tensor) and image.is_cuda and image.dim() == 4):
            raise ValueError("image: expected a CUDA tensor (F,3,S,S) (HIP kernels only, no CPU path)")
        F_ = image.shape[0]
        if not centres(F_, self.n_frame, self.border):
            raise ValueError(f"image: {F_} frames hold no centre of a window of n_frame = {self.n_frame} (border {self.border!r})")
        self.reset(word_id, total=F_)
        if meta is not None:
            self._upload_meta(meta, F_, image.shape[-1], image.device)      # (once, before any of the video's kernels is queued)
            self._meta_all = True
        parts = []
        for i0 in range(0, F_, self.chunk):
            parts.append(self.push(image[i0:i0 + self.chunk]))
        parts.append(self.flush())
        res = VideoResult.cat(parts)
        if self.topk is not None:
            res = self.fuse(res)
        return self.link(res) if self._link is not None else res

    def tube_stream(self, lag: int = 16) -> "TubeStream":
        """A ``TubeStream`` with this grounder's ``link``, ``n_frame`` and ``topk``: feed it the parts that ``push`` / ``flush`` return
        and drop them; fused choices and tube boxes come back while the frames arrive."""
        if self._link is None:
            raise ValueError("tube_stream: the grounder was built without link")
        return TubeStream(self._link, self.n_frame, lag)


# ---- streaming fusion and tube linking -------------------------------------------------------------------
@dataclass
class FuseChunk:
    """The temporally fused choice of m centres that became final: ``centres`` (m,), ``best`` (Q,m) int64, ``fused`` (Q,m,k),
    ``fused_boxes`` (Q,m,4) — the values of ``VideoGrounder.fuse`` on the whole run, bit for bit."""
    centres: torch.Tensor
    best: torch.Tensor
    fused: torch.Tensor
    fused_boxes: torch.Tensor


@dataclass
class TubeChunk:
    """The part of the track that a call released: ``centres`` (m,), ``tube`` (Q,m) int64 (candidate index per centre), ``tube_boxes``
    (Q,m,4); m may be 0.  ``fused``: the ``FuseChunk`` of the same call (other centres: fusion and linking trail the arrivals by
    different amounts), or None.  ``tube_score`` (Q,): set by ``flush`` only."""
    centres: torch.Tensor
    tube: torch.Tensor
    tube_boxes: torch.Tensor
    fused: Optional[FuseChunk] = None
    tube_score: Optional[torch.Tensor] = None


def fuse_delay(n_frame: int) -> int:
    """Centres that the fusion trails the arrivals by: centre b is final once centre b + n_frame - 1 - n_frame // 2 has arrived."""
    K = _check_window(n_frame)
    return K - 1 - K // 2


def stream_counts(arrived: int, n_frame: int, lag: int, fused_unary: bool, flushed: bool = False) -> Tuple[int, int, int]:
    """(fused, linked, released) after ``arrived`` centres: how many centres have their final fused scores, how many the Viterbi
    recursion has taken, how many tube entries are out.  Counts alone decide what a call hands out: nothing asks the device."""
    d = 0 if flushed else fuse_delay(n_frame)
    n_fused = max(0, arrived - d)
    linked = n_fused if fused_unary else arrived
    return n_fused, linked, linked if flushed else max(0, linked - lag)


def _check_lag(lag) -> int:
    if not isinstance(lag, int) or isinstance(lag, bool) or not 1 <= lag <= 64:
        raise ValueError(f"lag = {lag!r}: frames a streamed track trails the newest one, an int in 1 ... 64")
    return lag


def _check_stream_part(part, qk: Optional[Tuple[int, int]], where: str, need_keep: bool) -> Tuple[int, int, int]:
    """(Q, m, k) of a part of a stream; ValueError if it has no candidates, differs from the (Q, k) of the first part, or is not on
    the GPU."""
    if part.cand_feats is None or part.cand_scores is None or part.cand_boxes is None:
        raise ValueError(f"{where}: the part carries no candidates (the grounder was built without topk)")
    if need_keep and part.cand_keep is None:
        raise ValueError(f"{where}: the part carries no candidates of a grounder with link (cand_keep is None)")
    Q, m, k = part.cand_scores.shape
    if qk is not None and (Q, k) != tuple(qk):
        raise ValueError(f"{where}: the part has Q = {Q} queries of k = {k} candidates, the stream began with Q = {qk[0]}, k = {qk[1]}")
    if tuple(part.cand_boxes.shape) != (Q, m, k, 4) or tuple(part.cand_feats.shape[:3]) != (Q, m, k) or part.centres.numel() != m:
        raise ValueError(f"{where}: cand_boxes / cand_feats / centres do not match cand_scores {(Q, m, k)}")
    if not all(t.is_cuda for t in (part.cand_feats, part.cand_scores, part.cand_boxes, part.centres)):
        raise ValueError(f"{where}: expected CUDA tensors (HIP kernels only, no CPU path)")
    return Q, m, k


def _own(t: torch.Tensor) -> torch.Tensor:
    """A slice kept between calls owns its memory (a view would hold the whole staging tensor)."""
    return t.clone(memory_format=torch.contiguous_format)


def _nbytes(ts) -> int:
    return sum(t.numel() * t.element_size() for t in ts if t is not None)


class FuseStream:
    """``VideoGrounder.fuse`` while the centres arrive.  ``push(part)`` takes the next part of a stream (any number of centres, or
    None) and returns the centres that became final; ``flush()`` returns the last ``fuse_delay(n_frame)`` ones.  Between calls it
    keeps the candidates of the last n_frame - 1 centres.  Each call runs ``ops.post_fusion_bank`` on [kept | new] and takes the
    centres whose whole window lies inside (the start of the video and, at ``flush``, its end are the true borders): the same kernel
    on the same window contents as a run over the whole video."""

    def __init__(self, n_frame: int):
        self.n_frame = _check_window(n_frame)
        if n_frame > 32:
            raise ValueError(f"n_frame = {n_frame}: the temporal fusion takes n_frame <= 32")
        self._kept = None                  # (centres (s,), feats (Q,s,k,E), scores (Q,s,k), boxes (Q,s,k,4)) of the last s <= K - 1 centres
        self._qk = None
        self._n = self._done = 0           # centres arrived / handed out

    def state_bytes(self) -> int:
        return _nbytes(self._kept or ())

    def _emit(self, stage, hi: int) -> Optional[FuseChunk]:
        from . import ops
        cen, feats, scores, boxes = stage
        s0, lo = self._n - cen.numel(), self._done
        if hi <= lo:
            return None
        best, fused = zip(*[ops.post_fusion_bank(feats[q], scores[q], self.n_frame) for q in range(feats.shape[0])])
        best, fused = torch.stack(best)[:, lo - s0:hi - s0], torch.stack(fused)[:, lo - s0:hi - s0]
        fb = torch.gather(boxes[:, lo - s0:hi - s0], 2, best[:, :, None, None].expand(-1, -1, 1, 4))[:, :, 0]
        self._done = hi
        return FuseChunk(centres=cen[lo - s0:hi - s0], best=best, fused=fused, fused_boxes=fb)

    @torch.no_grad()
    def push(self, part: Optional[VideoResult]) -> Optional[FuseChunk]:
        if part is None:
            return None
        Q, m, k = _check_stream_part(part, self._qk, "FuseStream.push", False)
        self._qk = (Q, k)
        new = (part.centres, part.cand_feats.float(), part.cand_scores.float(), part.cand_boxes.float())
        dims = (0, 1, 1, 1)
        stage = tuple(t.contiguous() for t in new) if self._kept is None else \
            tuple(torch.cat([a, b], dim=d) for a, b, d in zip(self._kept, new, dims))
        self._n += m
        out = self._emit(stage, self._n - fuse_delay(self.n_frame))
        s = min(self.n_frame - 1, stage[0].numel())
        self._kept = tuple(_own(t.narrow(d, t.shape[d] - s, s)) for t, d in zip(stage, dims))
        return out

    @torch.no_grad()
    def flush(self) -> Optional[FuseChunk]:
        out = None if self._kept is None else self._emit(self._kept, self._n)
        self._kept, self._qk, self._n, self._done = None, None, 0, 0
        return out


class TubeStream:
    """``VideoGrounder.fuse`` and ``VideoGrounder.link`` while the centres arrive, with constant state.

        ts = vg.tube_stream(lag=16)                    # or TubeStream(TubeLink(), n_frame, lag)
        for frames in video: chunk = ts.push(vg.push(frames)); ...        # the part can be dropped at once
        ts.push(vg.flush()); last = ts.flush()

    ``push`` hands a centre's tube entry out once the Viterbi recursion is ``lag`` centres past it (for ``unary == "fused"`` the
    recursion itself trails the arrivals by ``fuse_delay(n_frame)``); ``flush`` hands out the rest and ``tube_score``.  How many
    centres a call releases follows from counts alone (``stream_counts``): nothing here synchronises the host with the device.
    ``forced`` (Q,) int32, a device tensor: how often a frame had to be committed although the live survivors disagreed on it.  While
    it is 0 the track is bit for bit that of ``link`` on the whole video."""

    def __init__(self, link: TubeLink, n_frame: int, lag: int = 16):
        if not isinstance(link, TubeLink):
            raise TypeError(f"link: expected a dcnet_amd.video.TubeLink, got {type(link).__name__}")
        self.link, self.n_frame, self.lag = link, _check_window(n_frame), _check_lag(lag)
        self._fs = FuseStream(n_frame)
        self._reset()

    def _reset(self):
        self._qk = None
        self._t = 0                        # centres the recursion has taken
        self._pend = None                  # (centres, boxes, feats, keep, scores) of the centres that wait for their fused scores
        self._last = None                  # (boxes (Q,1,k,4), feats (Q,1,k,E)) of centre _t - 1
        self._ring = None                  # (centres, boxes) of the centres [max(0, _t - lag), _t): not released yet
        self._delta = self._surv = None
        self.forced = None

    def state_bytes(self) -> int:
        """Bytes of the device tensors held between calls."""
        held = [self._delta, self._surv, self.forced]
        for group in (self._pend, self._last, self._ring):
            held.extend(group or ())
        return _nbytes(held) + self._fs.state_bytes()

    def _advance(self, r: int, unary: torch.Tensor):
        """The recursion over the first r waiting centres; returns (centres, tube, tube_boxes) of the frames it committed."""
        from . import ops
        cfg, lag, T = self.link, self.lag, self._t
        cen, boxes, feats, keep, _ = (t[:r] if i == 0 else t[:, :r] for i, t in enumerate(self._pend))
        use_feats = cfg.feat_weight > 0
        if T:
            sb = torch.cat([self._last[0], boxes], dim=1)
            sf = torch.cat([self._last[1], feats], dim=1) if use_feats else None
            W = ops.tube_transitions(sb, sf, 1, 1 + r, cfg.iou_weight, cfg.feat_weight)
        else:
            W = ops.tube_transitions(boxes.contiguous(), feats.contiguous() if use_feats else None, 0, r, cfg.iou_weight, cfg.feat_weight)
        commit = ops.tube_stream_step(W, unary.contiguous(), keep.contiguous(), T, lag, self._delta, self._surv, self.forced)
        rc, rb = (cen, boxes) if self._ring is None else (torch.cat([self._ring[0], cen]), torch.cat([self._ring[1], boxes], dim=1))
        lo, hi = max(0, T - lag), max(0, T + r - lag)                      # the ring begins at centre lo; [lo, hi) leave
        tube = commit[:, r - (hi - lo):]
        tb = torch.gather(rb[:, :hi - lo], 2, tube[:, :, None, None].expand(-1, -1, 1, 4))[:, :, 0]
        out = (rc[:hi - lo], tube, tb)
        self._ring = (_own(rc[hi - lo:]), _own(rb[:, hi - lo:]))
        self._last = (_own(boxes[:, r - 1:r]), _own(feats[:, r - 1:r]) if use_feats else None)
        rest = self._pend[0].numel() - r
        self._pend = tuple(_own(t[r:] if i == 0 else t[:, r:]) for i, t in enumerate(self._pend)) if rest else None
        self._t = T + r
        return out

    def _take(self, part: VideoResult, Q: int, k: int):
        dev = part.cand_scores.device
        if self._delta is None:
            self._delta = torch.empty((Q, k), dtype=torch.float32, device=dev)
            self._surv = torch.zeros((Q, self.lag, k), dtype=torch.uint8, device=dev)
            self.forced = torch.zeros(Q, dtype=torch.int32, device=dev)
        keep = part.cand_keep
        keep = keep.view(torch.uint8) if keep.dtype == torch.bool else keep
        new = (part.centres, part.cand_boxes.float(), part.cand_feats.float(), keep, part.cand_scores.float())
        self._pend = new if self._pend is None else tuple(torch.cat([a, b], dim=0 if i == 0 else 1)
                                                          for i, (a, b) in enumerate(zip(self._pend, new)))

    @torch.no_grad()
    def push(self, part: Optional[VideoResult]) -> Optional[TubeChunk]:
        """The next part of the stream (what ``VideoGrounder.push`` / ``flush`` returned; None: nothing).  Returns the fused choices
        and tube entries that this part completed, or None."""
        if part is None:
            return None
        Q, m, k = _check_stream_part(part, self._qk, "TubeStream.push", True)
        self._qk = (Q, k)
        fchunk = self._fs.push(part)
        self._take(part, Q, k)
        if self.link.unary == "fused":
            r, unary = (0, None) if fchunk is None else (fchunk.fused.shape[1], fchunk.fused)
        else:
            r, unary = m, self._pend[4]
        out = self._advance(r, unary) if r else None
        if out is None and fchunk is None:
            return None
        if out is None:
            dev = part.cand_scores.device
            out = (part.centres[:0], torch.empty((Q, 0), dtype=torch.int64, device=dev), torch.empty((Q, 0, 4), device=dev))
        return TubeChunk(centres=out[0], tube=out[1], tube_boxes=out[2], fused=fchunk)

    @torch.no_grad()
    def flush(self) -> Optional[TubeChunk]:
        """End of the stream: the centres not released yet and ``tube_score``; None if no centre ever arrived.  The stream is empty
        afterwards; ``forced`` keeps the count of the finished stream until the next ``push``."""
        from . import ops
        fchunk = self._fs.flush()
        outs = []
        if self._pend is not None:                                         # (unary "fused": the centres that waited for the end)
            outs.append(self._advance(self._pend[0].numel(), fchunk.fused))
        if not self._t:
            self._reset()
            return None
        tail, score = ops.tube_stream_flush(self._delta, self._surv, self._t, self.lag)
        rc, rb = self._ring
        outs.append((rc, tail, torch.gather(rb, 2, tail[:, :, None, None].expand(-1, -1, 1, 4))[:, :, 0]))
        cen, tube, tb = (torch.cat([o[i] for o in outs], dim=0 if i == 0 else 1) for i in range(3))
        forced = self.forced
        self._reset()
        self.forced = forced
        return TubeChunk(centres=cen, tube=tube, tube_boxes=tb, fused=fchunk, tube_score=score)


# ---- command line -------------------------------------------------------------------------------------------------------------
def synthetic_model(size: int, device):
    """The product model with the deterministic synthetic weights the tests and bench.py use (needs the repository's
    tests/golden/state_dict_keys_256.json and bn_calib.npz)."""
    import json
    from .model import grounding_model
    from .utils.synth import apply_bn_calibration, synth_state_dict
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    gold = os.path.join(root, "tests", "golden")
    with open(os.path.join(gold, "state_dict_keys_256.json")) as f:
        shapes = {k: tuple(v) for k, v in json.load(f).items()}
    shapes["loc_text_embedding.0.weight"] = (512, sum((size // 32 * 2 ** i) ** 2 for i in range(3)))
    sd = apply_bn_calibration(synth_state_dict(shapes, 0), os.path.join(gold, "bn_calib.npz"))
    m = grounding_model(corpus=list(range(1000)), light=False, emb_size=512, coordmap=True, dataset="vid", img_size=size,
                        config_path=os.path.join(root, "model", "yolov3.cfg"), weights_path=None)
    m.load_state_dict(sd, strict=True)
    return m.to(device).eval()


def main(argv=None):
    import argparse
    ap = argparse.ArgumentParser(description="whole-video grounding on synthetic frames")
    ap.add_argument("--synthetic", action="store_true", help="synthetic weights and frames (the only source this tool has)")
    ap.add_argument("--frames", type=int, default=64)
    ap.add_argument("--n-frame", type=int, default=5)
    ap.add_argument("--size", type=int, default=416)
    ap.add_argument("--border", default="valid", choices=BORDERS)
    ap.add_argument("--chunk", type=int, default=32)
    ap.add_argument("--queries", type=int, default=1)
    ap.add_argument("--topk", type=int, default=None)
    ap.add_argument("--link", action="store_true", help="link the top-k candidates into one track per query (needs --topk); prints the tube boxes")
    ap.add_argument("--stream-tubes", action="store_true", help="with --link: push the video chunk by chunk through a TubeStream, keep no part; prints the tube boxes as they are released")
    ap.add_argument("--lag", type=int, default=16, help="--stream-tubes: centres a tube entry trails the newest one (1 ... 64)")
    ap.add_argument("--raw-frames", action="store_true", help="375x500 uint8 frames through prep.prepare_clips(augment=False); prints source-pixel boxes")
    ap.add_argument("--repeat", type=int, default=3)
    ap.add_argument("--precision", default="fp32", choices=sorted(BANK_BYTES_PER_VALUE), help="ops.set_precision mode of the run")
    a = ap.parse_args(argv)
    if not a.synthetic:
        ap.error("only --synthetic input is built in; use VideoGrounder from Python for real videos")
    from . import ops
    ops.set_precision(a.precision)                   # (before the model is built; "fp32" again at the end)
    try:
        _main_run(a)
    finally:
        ops.set_precision("fp32")


def _main_run(a):
    import time
    import numpy as np
    from .utils.synth import synth_inputs
    dev = torch.device("cuda:0")
    m = synthetic_model(a.size, dev)
    image, word_id, _ = synth_inputs(a.frames, a.size, n_queries=a.queries, seed=1)
    meta = None
    if a.raw_frames:
        from . import prep
        rs = np.random.RandomState(7)
        frames = [[rs.randint(0, 256, size=(375, 500, 3)).astype(np.uint8) for _ in range(a.frames)]]
        p = prep.prepare_clips(frames, [np.tile(np.array([[10, 10, 100, 100]]), (a.frames, 1))], [["a phrase"] * a.frames], a.size, False)
        image, meta = p.image, (p.ratio, p.dw, p.dh)
    image, word_id = image.to(dev), word_id.to(dev)
    if a.link and a.topk is None:
        raise SystemExit("--link needs --topk")
    if a.stream_tubes and not a.link:
        raise SystemExit("--stream-tubes needs --link")
    vg = VideoGrounder(m, n_frame=a.n_frame, border=a.border, chunk=a.chunk, topk=a.topk, link=TubeLink() if a.link else None)
    if a.stream_tubes:
        return _main_stream(a, vg, image, word_id, meta)
    times = []
    for _ in range(a.repeat + 1):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        res = vg.run(image, word_id, meta)
        torch.cuda.synchronize()
        times.append(time.perf_counter() - t0)
    t = float(np.median(times[1:])) if len(times) > 1 else times[0]
    print(f"{a.frames} frames {a.size}x{a.size}, n_frame {a.n_frame}, border {a.border}, {a.queries} quer{'y' if a.queries == 1 else 'ies'}, "
          f"{a.precision}: {res.centres.numel()} centres in {t * 1e3:.1f} ms = {a.frames / t:.1f} frames/s, peak memory "
          f"{torch.cuda.max_memory_allocated() / 2 ** 30:.2f} GiB, bank {vg.bank_bytes_per_frame(a.size) / 2 ** 20:.2f} MiB per frame")
    if a.raw_frames or a.link:
        b = (res.tube_boxes if a.link else res.fused_boxes if a.topk is not None else res.boxes)[0].cpu()
        what = ("tube box" if a.link else "box") + (" (source pixels) " if a.raw_frames else " (letterbox pixels) ")
        for i, c in enumerate(res.centres.cpu().tolist()):
            print(f"frame {c}: {what}" + " ".join(f"{v:.1f}" for v in b[i].tolist()))
        if a.link:
            print(f"tube score {float(res.tube_score[0]):.4f}, candidates kept by the NMS: {float(res.cand_keep[0].float().sum(-1).mean()):.1f} of {a.topk} per centre")


def _main_stream(a, vg, image, word_id, meta):
    """--stream-tubes: every part goes to the TubeStream and is dropped.  The first pass (untimed) prints the tube boxes as they are
    released; the timed passes keep only the released chunks."""
    import time
    import numpy as np
    what = "tube box" + (" (source pixels) " if a.raw_frames else " (letterbox pixels) ")

    def one_pass(show: bool):
        vg.reset(word_id, total=a.frames)
        ts = vg.tube_stream(a.lag)
        n_out, peak_state, last = 0, 0, None
        parts = list(range(0, a.frames, a.chunk)) + [None]
        for i0 in parts:
            if i0 is None:
                part = vg.flush()
            else:
                part = vg.push(image[i0:i0 + a.chunk], None if meta is None else tuple(x[i0:i0 + a.chunk] for x in meta))
            chunks = [ts.push(part)]
            del part
            peak_state = max(peak_state, ts.state_bytes())
            if i0 is None:
                chunks.append(ts.flush())
            for ch in chunks:
                if ch is None:
                    continue
                last = ch
                n_out += ch.centres.numel()
                if show:
                    for c, b in zip(ch.centres.cpu().tolist(), ch.tube_boxes[0].cpu().tolist()):
                        print(f"frame {c}: {what}" + " ".join(f"{v:.1f}" for v in b))
        return n_out, peak_state, last, ts.forced

    times = []
    for r in range(a.repeat + 1):
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        t0 = time.perf_counter()
        n_out, state, last, forced = one_pass(show=r == 0)
        torch.cuda.synchronize()
        times.append(time.perf_counter() - t0)
    t = float(np.median(times[1:])) if len(times) > 1 else times[0]
    print(f"{a.frames} frames {a.size}x{a.size}, n_frame {a.n_frame}, border {a.border}, {a.queries} quer{'y' if a.queries == 1 else 'ies'}, "
          f"{a.precision}, streamed tubes (lag {a.lag}): {n_out} centres in {t * 1e3:.1f} ms = {a.frames / t:.1f} frames/s, peak memory "
          f"{torch.cuda.max_memory_allocated() / 2 ** 30:.2f} GiB, stream state {state / 2 ** 20:.2f} MiB")
    print(f"tube score {float(last.tube_score[0]):.4f}, forced {forced.cpu().tolist()}")


if __name__ == "__main__":
    main()
