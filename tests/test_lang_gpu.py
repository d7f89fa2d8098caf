"""The small language-branch kernels (embedding, row lengths, column sums, LSTM cell), the per-step recurrence built from them,
the persistent BiLSTM at its shortest sequences, and RNNEncoder on zero-padded queries, each against a plain fp64 (or, where the
kernel fixes its summation order, bitwise fp32) reference on the CPU."""
import pytest
import torch

from util import build_product, close, maxdiff, rand, synth_sd

pytestmark = pytest.mark.gpu

U = 2.0 ** -24          # one unit of fp32 rounding


def _below(got, ref64, bound64, name):
    """|got - ref64| <= bound64 element by element (fp64, CPU); where the bound is 0 the value is exactly the reference"""
    d = (got.detach().double().cpu() - ref64).abs()
    over = d - bound64
    worst = float((d / bound64.clamp_min(1e-300)).max()) if bool((bound64 > 0).any()) else 0.0
    print(f"LANGERR {name} worst err/bound {worst:.3f}")
    assert bool((over <= 0).all()), f"{name}: worst err / bound = {worst:.3f}, max excess {float(over.max()):.3e}"


# ---- embedding ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("e", [4, 512, 516])
def test_embedding_fwd_copies_table_rows_bitwise(dev, e):
    from dcnet_amd import ops
    vocab = 11
    table = rand(vocab, e, seed=1)
    g = torch.Generator().manual_seed(2)
    ids = torch.randint(0, vocab, (3, 14), generator=g)
    ids[0, 3], ids[2, 5] = -1, vocab                                    # out of range on either side: zero rows
    want = torch.zeros(3, 14, e)
    ok = (ids >= 0) & (ids < vocab)
    want[ok] = table[ids[ok]]
    td = table.to(dev)
    assert torch.equal(ops.embedding_fwd(ids.to(dev), td).cpu(), want)
    assert torch.equal(ops.embedding_fwd(ids.to(torch.int32).to(dev), td).cpu(), want)
    wide = torch.stack([ids, ids + 1], 2).to(dev)[:, :, 0]               # a non-contiguous view of the same ids
    assert not wide.is_contiguous()
    assert torch.equal(ops.embedding_fwd(wide, td).cpu(), want)
    small = ids.clamp(0, vocab)                                          # uint8 holds no -1
    want8 = torch.zeros(3, 14, e)
    ok8 = small < vocab
    want8[ok8] = table[small[ok8]]
    assert torch.equal(ops.embedding_fwd(small.to(torch.uint8).to(dev), td).cpu(), want8)


@pytest.mark.parametrize("e", [4, 516])
def test_embedding_bwd_sums_tokens_in_ascending_order(dev, e):
    from dcnet_amd import ops
    vocab, tokens = 13, 96
    g = torch.Generator().manual_seed(3)
    ids = torch.randint(0, vocab - 2, (tokens,), generator=g)            # rows vocab-2, vocab-1 stay unused
    ids[torch.randperm(tokens, generator=g)[:50]] = 5                    # one id 50 times
    ids[7], ids[40] = -1, vocab                                          # ignored
    dout = rand(tokens, e, seed=4)
    want32 = torch.zeros(vocab, e)
    for t in range(tokens):                                              # the kernel's order, one fp32 addition per token
        v = int(ids[t])
        if 0 <= v < vocab:
            want32[v] = want32[v] + dout[t]
    ok = (ids >= 0) & (ids < vocab)
    want64 = torch.zeros(vocab, e, dtype=torch.float64).index_add_(0, ids[ok], dout[ok].double())
    abs64 = torch.zeros(vocab, e, dtype=torch.float64).index_add_(0, ids[ok], dout[ok].double().abs())
    ids2d, dout2d = ids.view(8, 12).to(dev), dout.view(8, 12, e).to(dev)
    got = ops.embedding_bwd(ids2d, dout2d, vocab)
    again = ops.embedding_bwd(ids2d, dout2d, vocab)
    assert torch.equal(got, again), "two runs differ"
    assert torch.equal(got.cpu(), want32), maxdiff(got, want32)
    assert int((ids == 5).sum()) >= 50 and bool((got[vocab - 2:] == 0).all())
    _below(got, want64, tokens * U * abs64, f"embedding_bwd e={e}")


# ---- row lengths, column sums ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 256, 257])
@pytest.mark.parametrize("L", [1, 20])
def test_row_lengths_counts_nonzero_ids(dev, n, L):
    from dcnet_amd import ops
    g = torch.Generator().manual_seed(10 * n + L)
    ids = torch.randint(-3, 6, (n, L), generator=g)                      # zeros anywhere in a row, negative ids as well
    ids[n // 2] = 0                                                      # an all-zero row
    if L > 2 and n > 1:
        ids[0] = 7; ids[0, L // 2] = 0                                   # a zero in the middle is not counted
        ids[n - 1] = -1                                                  # negative ids count as non-zero
    want = (ids != 0).sum(1)
    got = ops.row_lengths(ids.to(dev))
    assert got.dtype == torch.int64 and torch.equal(got.cpu(), want)
    assert int(got[n // 2]) == 0
    if L > 2 and n > 1:
        assert int(got[0]) == L - 1 and int(got[n - 1]) == L
    assert torch.equal(ops.row_lengths(ids.to(torch.int32).to(dev)).cpu(), want)


@pytest.mark.parametrize("rows", [1, 7, 8, 9, 60])
@pytest.mark.parametrize("cols", [1, 255, 257])
def test_colsum_adds_rows_in_order(dev, rows, cols):
    from dcnet_amd import ops
    wide = rand(rows, cols + 5, seed=rows * 1000 + cols)
    x = wide[:, 2:2 + cols]                                              # row stride cols + 5
    want = torch.zeros(cols)
    for r in range(rows):
        want = want + x[r]
    got = ops.colsum(wide.to(dev)[:, 2:2 + cols])
    assert torch.equal(got.cpu(), want), maxdiff(got, want)
    assert torch.equal(ops.colsum(x.contiguous().to(dev)).cpu(), want)


@pytest.mark.parametrize("rows", [1, 255, 4099])
@pytest.mark.parametrize("c", [4, 512, 2048])
def test_rows_sum_against_fp64(dev, rows, c):
    from dcnet_amd import ops
    x = rand(rows, c, seed=rows + c)
    want, bound = x.double().sum(0), rows * U * x.double().abs().sum(0)
    _below(ops.rows_sum(x.to(dev)), want, bound, f"rows_sum {rows}x{c}")
    strided = torch.stack([x, x + 1], 1).to(dev)[:, 0]                   # colsum_rows takes any [rows][c] view
    assert not strided.is_contiguous() or rows == 1
    _below(ops.colsum_rows(strided), want, bound, f"colsum_rows {rows}x{c}")


# ---- LSTM cell ---------------------------------------------------------------------------------------------------------------
def _cell_ref(gates, c_prev, h_prev, live):
    """fp64 cell of fp32 inputs.  Returns the values and, for each, the sum of the absolute terms its fp32 evaluation rounds
    (|f.c_prev| + |i.g| for c, carried through tanh and the output gate): the scale of its error."""
    H = c_prev.shape[1]
    g64 = gates.double()
    i, f, g, o = torch.sigmoid(g64[:, :H]), torch.sigmoid(g64[:, H:2 * H]), torch.tanh(g64[:, 2 * H:3 * H]), torch.sigmoid(g64[:, 3 * H:])
    cp, hp = c_prev.double(), h_prev.double()
    c = f * cp + i * g
    sc = (f * cp).abs() + (i * g).abs()
    tc = torch.tanh(c)
    stc = tc.abs() + (1 - tc * tc) * sc
    h, sh = o * tc, o * stc
    lv = live.view(-1, 1)
    zero = torch.zeros_like(c)
    return {"act": (torch.cat([i, f, g, o, tc], 1), torch.cat([i, f, g.abs(), o, stc], 1)),
            "c_out": (torch.where(lv, c, cp), torch.where(lv, sc, zero)),
            "h_out": (torch.where(lv, h, hp), torch.where(lv, sh, zero)),
            "y": (torch.where(lv, h, zero), torch.where(lv, sh, zero))}


CELL_UNITS = 8          # roundings budgeted per element: a handful of fp32 operations plus expf / tanhf


@pytest.mark.parametrize("H", [8, 512])
@pytest.mark.parametrize("n", [1, 5, 70])
@pytest.mark.parametrize("masked", [False, True])
def test_lstm_cell_against_fp64(dev, H, n, masked):
    """Every output of dcn_lstm_cell_fwd / _bwd.  masked: rows alternate between t == len - 1 (live) and t == len (passed through:
    y and dgates zero, state and its gradients handed on unchanged); otherwise lens is None.  y, dy and dgates are column slices of
    wider buffers (ldy = 2H); the backward also runs with dh_rec and dc_next absent."""
    from dcnet_amd import ops
    s = 100 * H + n
    t = 3
    gates, c_prev, h_prev = rand(n, 4 * H, seed=s, scale=2.0), rand(n, H, seed=s + 1), rand(n, H, seed=s + 2)
    lens = torch.tensor([t + 1 if r % 2 == 0 else t for r in range(n)]) if masked else None
    live = torch.ones(n, dtype=torch.bool) if lens is None else t < lens
    ref = _cell_ref(gates, c_prev, h_prev, live)
    lens_d = None if lens is None else lens.to(dev)
    act = torch.empty(n, 5 * H, device=dev); c_out = torch.empty(n, H, device=dev); h_out = torch.empty(n, H, device=dev)
    ybuf = torch.full((n, 2 * H), -5.0, device=dev)
    y = ybuf[:, H:]
    ops.lstm_cell_fwd(gates.to(dev), c_prev.to(dev), h_prev.to(dev), lens_d, t, act, c_out, h_out, y)
    got = {"act": act, "c_out": c_out, "h_out": h_out, "y": y}
    for k, (val, scale) in ref.items():
        _below(got[k], val, CELL_UNITS * U * scale, f"cell_fwd {k} H={H} n={n} masked={masked}")
    assert bool((ybuf[:, :H] == -5.0).all())
    if masked:
        dead = ~live
        assert torch.equal(c_out.cpu()[dead], c_prev[dead]) and torch.equal(h_out.cpu()[dead], h_prev[dead])
        assert bool((y.cpu()[dead] == 0).all())
    # backward, from the activations the forward saved (fp32 values, evaluated in fp64)
    a64 = act.cpu().double()
    i, f, g, o, tc = (a64[:, j * H:(j + 1) * H] for j in range(5))
    dy, dhr, dcn = rand(n, H, seed=s + 3), rand(n, H, seed=s + 4), rand(n, H, seed=s + 5)
    for have in (True, False):
        r64 = dhr.double() if have else torch.zeros(n, H, dtype=torch.float64)
        n64 = dcn.double() if have else torch.zeros(n, H, dtype=torch.float64)
        dh, sdh = dy.double() + r64, dy.double().abs() + r64.abs()
        dc = n64 + dh * o * (1 - tc * tc)
        sdc = n64.abs() + sdh * o * (1 + tc * tc)
        want = {"dgates": (torch.cat([dc * g * i * (1 - i), dc * c_prev.double() * f * (1 - f), dc * i * (1 - g * g), dh * tc * o * (1 - o)], 1),
                           torch.cat([sdc * g.abs() * i * (1 + i), sdc * c_prev.double().abs() * f * (1 + f), sdc * i * (1 + g * g),
                                      sdh * tc.abs() * o * (1 + o)], 1)),
                "dc_prev": (dc * f, sdc * f), "dh_pass": (torch.zeros_like(dc), torch.zeros_like(dc))}
        lv = live.view(-1, 1)
        zero4 = torch.zeros(n, 4 * H, dtype=torch.float64)
        want["dgates"] = (torch.where(lv, want["dgates"][0], zero4), torch.where(lv, want["dgates"][1], zero4))
        want["dc_prev"] = (torch.where(lv, want["dc_prev"][0], n64), torch.where(lv, want["dc_prev"][1], torch.zeros_like(dc)))
        want["dh_pass"] = (torch.where(lv, want["dh_pass"][0], r64), want["dh_pass"][1])
        dybuf = rand(n, 2 * H, seed=s + 6).to(dev)
        dybuf[:, :H] = dy.to(dev)
        gbuf = torch.full((n, 8 * H), -5.0, device=dev)
        dgates = gbuf[:, 4 * H:]
        dc_prev = torch.empty(n, H, device=dev); dh_pass = torch.empty(n, H, device=dev)
        ops.lstm_cell_bwd(dybuf[:, :H], dhr.to(dev) if have else None, dcn.to(dev) if have else None, act, c_prev.to(dev), lens_d, t,
                          dgates, dc_prev, dh_pass)
        gotb = {"dgates": dgates, "dc_prev": dc_prev, "dh_pass": dh_pass}
        for k, (val, scale) in want.items():
            _below(gotb[k], val, CELL_UNITS * U * scale, f"cell_bwd {k} H={H} n={n} masked={masked} rec={have}")
        assert bool((gbuf[:, :4 * H] == -5.0).all())


# ---- recurrences ---------------------------------------------------------------------------------------------------------------
LSTM_FWD_TOL, LSTM_GRAD_TOL = 2e-5, 1e-4       # test_ops_gpu.test_bilstm_matches_torch_packed_lstm


def _lstm_weights(I, H, seed):
    k = 1.0 / H ** 0.5
    shapes = ((4 * H, I), (4 * H, H), (4 * H,), (4 * H,)) * 2
    return [(torch.rand(*s, generator=torch.Generator().manual_seed(seed + j)) * 2 - 1) * k for j, s in enumerate(shapes)]


def _bilstm_ref64(x, lens, params):
    """out (n, L, 2H), acts (2, n, L, 5H), cprev (2, n, L, H) in fp64: the recurrence of csrc/lstm.hip written out
    (activations are computed at every step, the state moves only where t < len)"""
    n, L, _ = x.shape
    H = params[1].shape[1]
    out = torch.zeros(n, L, 2 * H, dtype=torch.float64); acts = torch.zeros(2, n, L, 5 * H, dtype=torch.float64)
    cprev = torch.zeros(2, n, L, H, dtype=torch.float64)
    for d in range(2):
        w_ih, w_hh, b_ih, b_hh = (p.double() for p in params[4 * d:4 * d + 4])
        h = torch.zeros(n, H, dtype=torch.float64); c = torch.zeros(n, H, dtype=torch.float64)
        for t in (range(L) if d == 0 else range(L - 1, -1, -1)):
            g = x[:, t].double() @ w_ih.t() + b_ih + h @ w_hh.t() + b_hh
            i, f, gg, o = torch.sigmoid(g[:, :H]), torch.sigmoid(g[:, H:2 * H]), torch.tanh(g[:, 2 * H:3 * H]), torch.sigmoid(g[:, 3 * H:])
            cn = f * c + i * gg
            tc = torch.tanh(cn)
            acts[d, :, t] = torch.cat([i, f, gg, o, tc], 1); cprev[d, :, t] = c
            lv = (t < lens).view(-1, 1)
            out[:, t, d * H:(d + 1) * H] = torch.where(lv, o * tc, torch.zeros_like(c))
            h, c = torch.where(lv, o * tc, h), torch.where(lv, cn, c)
    return out, acts, cprev


def test_per_step_recurrence_matches_the_persistent_kernel(dev):
    """The path dcn_bilstm_fwd's residency error names: xg and h . W_hh^T through ops.gemm_nt (bias, and xg[:, t] as a residual
    with its own row stride), the gates through dcn_lstm_cell_fwd, y written straight into its column block of `out`."""
    from dcnet_amd import ops
    n, L, I, H = 5, 4, 512, 512
    lens = torch.tensor([4, 1, 3, 4, 2])
    x = rand(n, L, I, seed=40)
    params = _lstm_weights(I, H, 41)
    ref_out, ref_acts, ref_cprev = _bilstm_ref64(x, lens, params)
    pd = [p.to(dev) for p in params]
    lens_d = lens.to(dev)
    xg = torch.empty(2, n, L, 4 * H, device=dev)
    for d in range(2):
        ops.gemm_nt(x.to(dev).view(n * L, I), pd[4 * d], pd[4 * d + 2], out=xg[d].view(n * L, 4 * H))
    out_k, _, cprev_k, acts_k = ops.bilstm_fwd(xg, pd[1], pd[5], pd[3], pd[7], lens_d)
    out_s = torch.full((n, L, 2 * H), -5.0, device=dev); acts_s = torch.empty(2, n, L, 5 * H, device=dev)
    cprev_s = torch.empty(2, n, L, H, device=dev)
    for d in range(2):
        h = torch.zeros(n, H, device=dev); c = torch.zeros(n, H, device=dev)
        for t in (range(L) if d == 0 else range(L - 1, -1, -1)):
            gates = ops.gemm_nt(h, pd[4 * d + 1], pd[4 * d + 3], residual=xg[d][:, t])
            act = torch.empty(n, 5 * H, device=dev); c2 = torch.empty_like(c); h2 = torch.empty_like(h)
            ops.lstm_cell_fwd(gates, c, h, lens_d, t, act, c2, h2, out_s[:, t, d * H:(d + 1) * H])
            acts_s[d, :, t] = act; cprev_s[d, :, t] = c
            h, c = h2, c2
    assert not ops.bilstm_sync_error(dev)
    for name, step, kern, ref in (("out", out_s, out_k, ref_out), ("acts", acts_s, acts_k, ref_acts), ("cprev", cprev_s, cprev_k, ref_cprev)):
        print(f"LANGERR per-step {name}: step-kernel {maxdiff(step, kern):.3e} step-fp64 {maxdiff(step, ref):.3e} kernel-fp64 {maxdiff(kern, ref):.3e}")
        close(step, kern, 2 * LSTM_FWD_TOL, f"per-step vs persistent {name}")
        close(step, ref, LSTM_FWD_TOL, f"per-step vs fp64 {name}")
        close(kern, ref, LSTM_FWD_TOL, f"persistent vs fp64 {name}")
    dead = torch.arange(L)[None, :] >= lens[:, None]
    assert bool((out_s.cpu()[dead] == 0).all()) and bool((out_k.cpu()[dead] == 0).all())


@pytest.mark.parametrize("L,lengths", [(1, [1, 1, 1]), (2, [2, 2, 2]), (2, [2, 1, 2])])
def test_persistent_bilstm_at_one_and_two_steps(dev, L, lengths):
    """L = 1: no workgroup ever waits and hprev is never written; L = 2: exactly one hand-over.  Forward and backward against
    nn.LSTM on a packed batch in fp64."""
    from dcnet_amd import ops
    from dcnet_amd.functions import BiLSTM
    torch.manual_seed(5)
    n, I, H = 3, 512, 512
    ref = torch.nn.LSTM(I, H, 1, batch_first=True, bidirectional=True).double()
    x, g = rand(n, L, I, seed=50), rand(n, L, 2 * H, seed=51)
    lens = torch.tensor(lengths)
    xr = x.double().requires_grad_(True)
    yr, _ = ref(torch.nn.utils.rnn.pack_padded_sequence(xr, lens, batch_first=True, enforce_sorted=False))
    yr, _ = torch.nn.utils.rnn.pad_packed_sequence(yr, batch_first=True, total_length=L)
    (yr * g.double()).sum().backward()
    names = ["weight_ih_l0", "weight_hh_l0", "bias_ih_l0", "bias_hh_l0", "weight_ih_l0_reverse", "weight_hh_l0_reverse",
             "bias_ih_l0_reverse", "bias_hh_l0_reverse"]
    params = [getattr(ref, nm).detach().float().to(dev).requires_grad_(True) for nm in names]
    xd = x.to(dev).requires_grad_(True)
    y = BiLSTM.apply(xd, lens.to(dev), *params)
    (y * g.to(dev)).sum().backward()
    assert not ops.bilstm_sync_error(dev)
    close(y, yr, LSTM_FWD_TOL, "out"); close(xd.grad, xr.grad, LSTM_GRAD_TOL, "dx")
    for p, nm in zip(params, names):
        close(p.grad, getattr(ref, nm).grad, LSTM_GRAD_TOL, nm)


# ---- RNNEncoder on zero-padded queries -----------------------------------------------------------------------------------------------
VOCAB, QLEN = 50, 20


def _encoder(dev):
    from dcnet_amd.model import RNNEncoder
    torch.manual_seed(6)
    m = RNNEncoder(vocab_size=VOCAB, word_embedding_size=512, word_vec_size=512, hidden_size=512, bidirectional=True,
                   input_dropout_p=0.0, variable_lengths=True)
    return m.to(dev)


def _padded_ids(lengths, seed):
    g = torch.Generator().manual_seed(seed)
    ids = torch.randint(1, 9, (len(lengths), QLEN), generator=g)         # eight words over up to 120 places: repeated within and across rows
    for r, n in enumerate(lengths):
        ids[r, n:] = 0
    return ids


def _cotangents(n, seed):
    return rand(n, 1024, seed=seed), rand(n, QLEN, 1024, seed=seed + 1), rand(n, QLEN, 512, seed=seed + 2)


def _run_product(m, ids, cots, dev):
    m.zero_grad(set_to_none=True)
    outs = m(ids.to(dev))
    sum((o * c.to(dev)).sum() for o, c in zip(outs, cots)).backward()
    return [o.detach().cpu() for o in outs], {k: p.grad.detach().cpu().clone() for k, p in m.named_parameters()}


def _run_oracle(m, ids, cots):
    from oracle import dcnet_oracle as O
    sd = {k: v.detach().cpu().double().requires_grad_(True) for k, v in m.state_dict().items()}
    outs = O.rnn_encoder(sd, ids, training=False, p="")
    sum((o * c.double()).sum() for o, c in zip(outs, cots)).backward()
    return [o.detach() for o in outs], {k: v.grad for k, v in sd.items()}


def _compare(outs, grads, ref_outs, ref_grads, tag):
    for name, a, b in zip(("sent", "context", "embedded"), outs, ref_outs):
        print(f"LANGERR encoder {tag} {name} {maxdiff(a, b):.3e}")
        close(a, b, LSTM_FWD_TOL, f"{tag} {name}")
    assert len(grads) == len(ref_grads) == 11
    for k in grads:
        print(f"LANGERR encoder {tag} d{k} {maxdiff(grads[k], ref_grads[k]):.3e} of {float(ref_grads[k].abs().max()):.3e}")
        close(grads[k], ref_grads[k], LSTM_GRAD_TOL, f"{tag} d{k}")


def test_rnn_encoder_on_padded_queries_matches_the_oracle(dev):
    m = _encoder(dev)
    lengths = [20, 7, 20, 13, 1, 20]
    ids, cots = _padded_ids(lengths, 60), _cotangents(6, 61)
    outs, grads = _run_product(m, ids, cots, dev)
    ref_outs, ref_grads = _run_oracle(m, ids, cots)
    _compare(outs, grads, ref_outs, ref_grads, "ragged")
    assert bool((grads["embedding.weight"][0] == 0).all()), "the padding row of the table received a gradient"
    dead = torch.arange(QLEN)[None, :] >= torch.tensor(lengths)[:, None]
    assert bool((outs[1][dead] == 0).all()) and bool((outs[2][dead] == 0).all())


def test_rnn_encoder_when_no_row_is_full(dev):
    m = _encoder(dev)
    ids, cots = _padded_ids([9, 3, 1, 8], 62), _cotangents(4, 63)
    outs, grads = _run_product(m, ids, cots, dev)
    ref_outs, ref_grads = _run_oracle(m, ids[:, :9], (cots[0], cots[1][:, :9], cots[2][:, :9]))
    assert bool((outs[1][:, 9:] == 0).all()) and bool((outs[2][:, 9:] == 0).all())
    _compare([outs[0], outs[1][:, :9], outs[2][:, :9]], grads, ref_outs, ref_grads, "short")
    assert bool((grads["embedding.weight"][0] == 0).all())


def test_rnn_encoder_with_an_all_zero_row(dev):
    """The reference cannot run an empty query; the product must treat it as a row that contributes nothing."""
    m = _encoder(dev)
    ids, cots = _padded_ids([20, 5, 0, 12], 64), _cotangents(4, 65)
    keep = [0, 1, 3]
    outs, grads = _run_product(m, ids, cots, dev)
    outs3, grads3 = _run_product(m, ids[keep], [c[keep] for c in cots], dev)
    for o in outs:
        assert bool(torch.isfinite(o).all()) and bool((o[2] == 0).all())
    for gname, gval in grads.items():
        assert bool(torch.isfinite(gval).all()), gname
    _compare([o[keep] for o in outs], grads, outs3, grads3, "empty-row")
    assert bool((grads["embedding.weight"][0] == 0).all())


def test_whole_model_with_a_padded_query(dev):
    """test_model_gpu's smallest eval case (S256, N2) with the second query cut to 7 words and zero-padded, at that test's tolerance"""
    import random
    from dcnet_amd.utils.synth import synth_inputs
    from oracle import dcnet_oracle as O
    from test_model_gpu import TOL
    size, n = 256, 2
    sd = synth_sd(size)
    image, word_id, word_mask = synth_inputs(n, size, seed=size + n)
    word_id[1, 7:] = 0
    m = build_product(size, sd, dev).eval()
    random.seed(13)
    with torch.no_grad():
        outbox, sim, loc, only_obj = m(image.to(dev), word_id.to(dev), word_mask.to(dev))
        o = O.grounding_forward_pairs({k: v.clone() for k, v in sd.items()}, image, word_id, training=False, sample=False)
    for s in range(3):
        for name, a, b in (("outbox", outbox, o["outbox"]), ("sim", sim, o["sim_score"]), ("loc", loc, o["loc_score"]),
                           ("only_obj", only_obj, o["only_obj"])):
            d = maxdiff(a[s], b[s])
            print(f"LANGERR model padded {name}{s} {d:.3e}")
            assert d < TOL, (name, s, d)
