"""GPU: whole-video grounding on bf16 storage ("bf16s"): the bf16 bank writer and the concat pass of csrc/video.hip against the existing
fp32 kernels plus torch's cast, the co-attention form query, and VideoGrounder under "bf16s" against the windowed n_frame model of the
same mode.  The yardstick of the model-level tests is the mode itself: d_mode = |windowed bf16s - windowed fp32| on the same inputs, from
code that does not go through the bank path; the restructured path must stay below it.  Synthetic weights, one model per mode."""
import contextlib
import functools

import pytest
import torch

from util import build_product, maxdiff, synth_sd

pytestmark = pytest.mark.gpu
FIELDS = ("outbox", "sim", "loc", "corr_feat", "only_obj")


@contextlib.contextmanager
def _precision(mode):
    from dcnet_amd import ops
    outer = ops.get_precision()          # ("fp32" at the outermost level; nested blocks — a model built inside one — hand back the outer mode)
    ops.set_precision(mode)
    try:
        yield
    finally:
        ops.set_precision(outer)


@functools.lru_cache(maxsize=None)
def _model(mode):
    with _precision(mode):
        return build_product(256, synth_sd(256), torch.device("cuda:0"), test_model=True).eval()


@functools.lru_cache(maxsize=None)
def _inputs(frames, seed, queries=1):
    from dcnet_amd.utils.synth import synth_inputs
    image, word_id, _ = synth_inputs(frames, 256, n_queries=queries, seed=seed)
    return image.to("cuda:0"), word_id.to("cuda:0")


def _rand(*shape, seed=0):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed))


def _cat(ref):
    """list (per centre) of the n_frame model's tuples -> one tuple of per-scale lists with the centres as the batch"""
    return tuple([torch.cat([r[i][s] for r in ref]) for s in range(3)] for i in range(5))


@functools.lru_cache(maxsize=None)
def _windowed(mode, frames, seed, K, border, q=0, queries=1):
    """The n_frame model of ``mode``, one window per call (code that does not know the bank path), for every centre.  Computed once per
    argument set and shared; nobody writes to it."""
    from dcnet_amd import video as V
    image, word_id = _inputs(frames, seed, queries)
    out = []
    with _precision(mode), torch.no_grad():
        m = _model(mode)
        for i in V.centres(frames, K, border):
            out.append(m(image[V.window_frames(i, frames, K, border)].contiguous(), word_id[q:q + 1], None, K))
    return _cat(out)


def _diffs(a, b):
    return {f: max(maxdiff(x.reshape(y.shape), y) for x, y in zip(a[i], b[i])) for i, f in enumerate(FIELDS)}


def _d_mode(frames, seed, K, border, q=0, queries=1):
    return _diffs(_windowed("bf16s", frames, seed, K, border, q, queries), _windowed("fp32", frames, seed, K, border, q, queries))


def _run_b16(frames, seed, queries=1, **kw):
    from dcnet_amd import video as V
    image, word_id = _inputs(frames, seed, queries)
    with _precision("bf16s"):
        return V.VideoGrounder(_model("bf16s"), **kw).run(image, word_id)


def _bits(t):
    return t.contiguous().view(torch.int16 if t.element_size() == 2 else torch.int32)


# ---- 1 ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", ["split", "bank", "both"])
@pytest.mark.parametrize("rows", [111, 5, 1])
@pytest.mark.parametrize("c", [256, 512, 1024])
def test_bank_writer_b16(dev, c, rows, form):
    """rows16 bitwise bank_write's fp32 rows cast by torch (round to nearest even), split / bank bitwise bank_write's; 4 rows per block, so
    111, 5 and 1 rows end in partial blocks; a zero row gives zeros; dense x and x with a row stride.  Outputs are sentinel-filled with
    three guard rows behind them: what was not asked for, and the guard rows, keep the sentinel."""
    from dcnet_amd import ops
    wide = (_rand(rows, c + 32, seed=c + rows) * 3.0).to(dev)
    if rows > 1:
        wide[rows // 2] = 0.0
    for x in (wide[:, :c].contiguous(), wide[:, :c]):
        ref_bank = torch.empty(rows, c, device=dev); ref_split = torch.empty(rows, c, device=dev)
        ops.bank_write(x, ref_bank, ref_split)
        rows16 = torch.full((rows + 3, c), 7.0, dtype=torch.bfloat16, device=dev)
        bank = torch.full((rows + 3, c), 7.0, device=dev); split = torch.full((rows + 3, c), 7.0, device=dev)
        ops.bank_write_b16(x, rows16[:rows], bank=bank[:rows] if form in ("bank", "both") else None,
                           split=split[:rows] if form in ("split", "both") else None)
        assert torch.equal(_bits(rows16[:rows]), _bits(ref_bank.to(torch.bfloat16)))
        if rows > 1:
            assert float(rows16[rows // 2].float().abs().max()) == 0.0
        for name, got, want in (("bank", bank, ref_bank), ("split", split, ref_split)):
            if form in (name, "both"):
                assert torch.equal(_bits(got[:rows]), _bits(want)), name
            else:
                assert bool((got == 7.0).all()), f"{name} was not asked for"
            assert bool((got[rows:] == 7.0).all()), f"{name}: rows behind the end"
        assert bool((rows16[rows:] == 7.0).all())
    with pytest.raises(ValueError, match="rows16"):
        ops.bank_write_b16(wide[:, :c], torch.empty(rows, c, device=dev))                      # an fp32 tensor is no rows16
    with pytest.raises(ValueError, match="must hold"):
        ops.bank_write_b16(wide[:, :c], torch.empty(rows + 1, c, dtype=torch.bfloat16, device=dev))


# ---- 2 ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", [256, 512])
@pytest.mark.parametrize("hw", [64, 169])
def test_bank_concat_b16(dev, hw, c):
    """[rows16[a0:a0 + n] | bf16(attn)] of a 6-frame bank, a0 = 2, n = 3: bitwise torch.cat of the rows and torch's cast, for attn dense
    and attn as the upper half of a (n, hw, 2c) fp32 tensor (the strides coattn_bank_fwd writes with in fp32); the frame behind the
    result keeps its sentinel."""
    from dcnet_amd import ops
    nf, a0, n = 6, 2, 3
    rows16 = _rand(nf, hw, c, seed=hw + c).to(torch.bfloat16).to(dev)
    wide = (_rand(n, hw, 2 * c, seed=hw + c + 1) * torch.logspace(-6, 3, 2 * c)).to(dev)         # values over nine decades
    for attn in (wide[..., c:].contiguous(), wide[..., c:]):
        want = torch.cat([rows16[a0:a0 + n], attn.to(torch.bfloat16)], -1)
        buf = torch.full((n + 1, hw, 2 * c), 7.0, dtype=torch.bfloat16, device=dev)
        got = ops.bank_concat_b16(rows16, a0, attn, cat=buf[:n])
        assert got.data_ptr() == buf.data_ptr() and torch.equal(_bits(got), _bits(want))
        assert bool((buf[n] == 7.0).all())
        assert torch.equal(_bits(ops.bank_concat_b16(rows16, a0, attn)), _bits(want))              # allocates its result
    with pytest.raises(ValueError, match="outside a bank"):
        ops.bank_concat_b16(rows16, 4, wide[..., c:])
    with pytest.raises(ValueError, match="attn"):
        ops.bank_concat_b16(rows16, a0, wide[..., c:].to(torch.bfloat16))


# ---- 3 ------------------------------------------------------------------------------------------------------------------------
def test_coattn_bank_form_and_single_operand_calls(dev):
    """Under "bf16s", c = 512: hw = 1024 runs on gemm3.hip (reads split), hw = 64 falls back (reads the fp32 rows).  coattn_bank_fwd with the
    tensor its form does not read left out is bitwise the call with both; with the one it reads left out it raises."""
    from dcnet_amd import ops
    c, nf = 512, 4
    with _precision("bf16s"):
        assert ops.coattn_bank_form(1024, c) == 1 and ops.coattn_bank_form(64, c) == 0
        for g in (32, 8):
            hw = g * g
            x = _rand(nf, hw, c, seed=g).to(dev)
            bank = torch.empty(nf, hw, c, device=dev); split = torch.empty_like(bank)
            ops.bank_write(x, bank, split)
            on3 = ops.coattn_bank_form(hw, c)
            both = torch.zeros(2, 3, hw, c, device=dev); one = torch.zeros(2, 3, hw, c, device=dev)
            ops.coattn_bank_fwd(bank, split, 0, 1, 3, both[0], both[1], 10.0)
            ops.coattn_bank_fwd(None if on3 else bank, split if on3 else None, 0, 1, 3, one[0], one[1], 10.0)
            assert torch.equal(one, both) and float(both.abs().max()) > 0
            with pytest.raises(ValueError, match="split is None" if on3 else "bank is None"):
                ops.coattn_bank_fwd(bank if on3 else None, None if on3 else split, 0, 1, 3, one[0], one[1], 10.0)
        with pytest.raises(ValueError, match="neither"):
            ops.coattn_bank_fwd(None, None, 0, 1, 3, one[0], one[1], 10.0)


# ---- 4 ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K", [5, 2])
def test_sliding_matches_the_windowed_path_b16(dev, K):
    """F = 12 at 256x256, one query, "bf16s": per field d_path = max |VideoGrounder - model(window_i, word_id, None, K)| (both on bf16
    storage) must be below d_mode = max |windowed bf16s - windowed fp32|: the two paths share every rounding point and differ only through
    the batch-shape-dependent summation order, which can flip an isolated bf16 rounding, whereas the mode rounds every element.
    Measured (MI355X), d_path / d_mode: K = 5 outbox 3.31e-2 / 1.15, sim 2.65e-5 / 2.04e-2, loc 6.41e-3 / 2.31e-1, corr_feat 9.95e-5 /
    6.48e-2, only_obj 1.43e-2 / 4.03e-1; K = 2 outbox 3.45e-2 / 1.24, sim 7.17e-5 / 2.38e-2, loc 5.33e-3 / 2.79e-1, corr_feat 2.84e-4 /
    6.66e-2, only_obj 1.61e-2 / 4.75e-1.  Outputs are fp32 and finite; the boxes of the result are decode_boxes of
    its own outbox (boxes are not compared across paths: an arg-max between near-tied cells may move)."""
    from dcnet_amd import losses
    from dcnet_amd import video as V
    res = _run_b16(12, 77, n_frame=K, border="valid")
    cs = V.centres(12, K, "valid")
    assert res.centres.tolist() == cs and res.boxes.shape == (1, len(cs), 4)
    d_path = _diffs(res.query(0), _windowed("bf16s", 12, 77, K, "valid"))
    d_mode = _d_mode(12, 77, K, "valid")
    for f in FIELDS:
        print(f"sliding bf16s K={K} {f}: d_path {d_path[f]:.3e}  d_mode {d_mode[f]:.3e}")
    for group in res.query(0):
        for t in group:
            assert t.dtype == torch.float32 and bool(torch.isfinite(t).all())
    assert torch.equal(res.boxes[0], losses.decode_boxes(res.query(0)[0], 256))
    for f in FIELDS:
        assert d_path[f] < d_mode[f], (K, f, d_path[f], d_mode[f])


# ---- 5 ------------------------------------------------------------------------------------------------------------------------
def test_chunked_streamed_and_repeatable_b16(dev):
    """"bf16s": a second run() is bitwise the first; push in chunks of 1 / 5 / 12 plus flush gives the same centres and every field within
    that field's d_mode of run()."""
    from dcnet_amd import video as V
    image, word_id = _inputs(12, 77)
    d_mode = _d_mode(12, 77, 5, "valid")
    with _precision("bf16s"):
        vg = V.VideoGrounder(_model("bf16s"), n_frame=5, border="valid")
        first = vg.run(image, word_id)
        again = vg.run(image, word_id)
        for a, b in zip(first.query(0), again.query(0)):
            assert all(torch.equal(x, y) for x, y in zip(a, b))
        assert torch.equal(first.boxes, again.boxes) and torch.equal(first.centres, again.centres)
        for chunk in (1, 5, 12):
            vg.reset(word_id)
            got = V.VideoResult.cat([vg.push(image[i:i + chunk]) for i in range(0, 12, chunk)] + [vg.flush()])
            assert got.centres.tolist() == first.centres.tolist()
            d = _diffs(got.query(0), first.query(0))
            print(f"push chunk {chunk}:", {k: f"{v:.2e}" for k, v in d.items()})
            for f in FIELDS:
                assert d[f] <= d_mode[f], (chunk, f, d[f], d_mode[f])


# ---- 6 ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("known_length", [True, False])
def test_replicate_border_b16(dev, known_length):
    """F = 6, K = 5, "bf16s": every frame is a centre (0, 1, 4, 5 with clamped windows), every field within d_mode of the windowed bf16s
    model on explicitly replicated frames."""
    from dcnet_amd import video as V
    image, word_id = _inputs(6, 55)
    with _precision("bf16s"):
        vg = V.VideoGrounder(_model("bf16s"), n_frame=5, border="replicate", chunk=4)
        if known_length:
            res = vg.run(image, word_id)
        else:
            vg.reset(word_id)
            res = V.VideoResult.cat([vg.push(image[:4]), vg.push(image[4:]), vg.flush()])
    assert res.centres.tolist() == list(range(6))
    d = _diffs(res.query(0), _windowed("bf16s", 6, 55, 5, "replicate"))
    d_mode = _d_mode(6, 55, 5, "replicate")
    for f in FIELDS:
        print(f"replicate bf16s known={known_length} {f}: d {d[f]:.3e}  d_mode {d_mode[f]:.3e}")
    for f in FIELDS:
        assert d[f] <= d_mode[f], (f, d[f], d_mode[f])


# ---- 7 ------------------------------------------------------------------------------------------------------------------------
def test_multi_query_and_topk_b16(dev):
    """"bf16s": 3 queries with chunk = 5, each within that query's d_mode of its single-query run; a topk = 4 run has sorted, finite
    candidate scores and fused_boxes = cand_boxes gathered at best."""
    from dcnet_amd import video as V
    image, word_id = _inputs(12, 78, 3)
    with _precision("bf16s"):
        vg = V.VideoGrounder(_model("bf16s"), n_frame=5, chunk=5)
        res = vg.run(image, word_id)
        singles = [vg.run(image, word_id[q]) for q in range(3)]
        top = V.VideoGrounder(_model("bf16s"), n_frame=5, topk=4).run(image, word_id[:1])
    for q in range(3):
        d = _diffs(res.query(q), singles[q].query(0))
        d_mode = _d_mode(12, 78, 5, "valid", q, 3)
        print(f"query {q}:", {k: f"{v:.2e} / {d_mode[k]:.2e}" for k, v in d.items()})
        for f in FIELDS:
            assert d[f] <= d_mode[f], (q, f, d[f], d_mode[f])
    assert maxdiff(res.outbox[0][0], res.outbox[1][0]) > 1e-3            # the queries do differ
    n = top.centres.numel()
    assert top.cand_scores.shape == (1, n, 4) and top.cand_boxes.shape == (1, n, 4, 4)
    assert bool(torch.isfinite(top.cand_scores).all()) and bool(torch.isfinite(top.cand_boxes).all())
    assert bool(torch.all(top.cand_scores[..., :-1] >= top.cand_scores[..., 1:]))
    assert torch.equal(top.fused_boxes[0], top.cand_boxes[0][torch.arange(n, device=dev), top.best[0]])


# ---- 8 ------------------------------------------------------------------------------------------------------------------------
def test_state_and_modes(dev):
    """Bank bytes per frame: 6 per value under "bf16s" (bf16 rows + split or fp32 rows, never both), 8 under "fp32" — by the public
    method and by the tensors the grounder actually keeps.  Modes without the path raise and name themselves; a mode change between reset
    and push raises; an fp32 run after a bf16s run is bitwise the fp32 run before it."""
    from dcnet_amd import ops
    from dcnet_amd import video as V
    image, word_id = _inputs(12, 77)
    values = sum(g * g for g in (8, 16, 32)) * 512
    vg32 = V.VideoGrounder(_model("fp32"), n_frame=5)
    before = vg32.run(image, word_id)
    assert vg32.bank_bytes_per_frame(256) == values * 8
    with _precision("bf16s"):
        vg = V.VideoGrounder(_model("bf16s"), n_frame=5)
        assert vg.bank_bytes_per_frame(256) == values * (2 + 4) < values * 8
        vg.reset(word_id)
        vg.push(image[:4])
        kept = [sum(t.element_size() * t[0].numel() for t in pair) for pair in vg._bank]
        assert [len(pair) for pair in vg._bank] == [2, 2, 2] and sum(kept) == vg.bank_bytes_per_frame()
        assert vg._form == [ops.coattn_bank_form(g * g, 512) for g in (8, 16, 32)] == [0, 0, 1]
        ops.set_precision("fp32")
        with pytest.raises(RuntimeError, match="bf16s"):
            vg.push(image[4:8])
        with pytest.raises(RuntimeError, match="bf16s"):
            vg.flush()
        ops.set_precision("bf16s")
        assert vg.push(image[4:8]) is not None
        vg.flush()
        mid = vg.run(image, word_id)
        assert bool(torch.isfinite(mid.boxes).all())
    for mode in ("bf16", "fp8s"):
        with _precision(mode):
            with pytest.raises(RuntimeError, match=repr(mode)):
                vg32.reset(word_id)
            with pytest.raises(RuntimeError, match=repr(mode)):
                vg32.bank_bytes_per_frame(256)
    after = vg32.run(image, word_id)
    for a, b in zip(before.query(0), after.query(0)):
        assert all(torch.equal(x, y) for x, y in zip(a, b))
    assert torch.equal(before.boxes, after.boxes)
