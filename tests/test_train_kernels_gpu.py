"""Direct float64 tests of the training-step entry points of csrc/train*.hip, called through capi.call at the shapes, strides and size
thresholds where their code paths change, plus the Adam drop-in against torch.optim.Adam.

Yardstick (tests/train_ref.py): |hip - f64| <= max(4 |torch_fp32 - f64|, atol + rtol |f64|) per element, with f64 the same operation in
float64 on the very fp32 inputs the kernel received and torch_fp32 torch's own fp32 evaluation of it; the element-wise ops are held to 4 fp32
ulps of the largest term that enters the element; row shuffles and grouped launches are bitwise.  Every output buffer starts as NaN or a
sentinel, so an element the kernel does not write fails."""
import numpy as np
import pytest
import torch

import train_ref as R

pytestmark = pytest.mark.gpu

SENT = 12345.0


def _gpu():
    if not torch.cuda.is_available():
        pytest.skip('no GPU')
    return torch.device('cuda:0')


def _capi():
    from sttode_amd import capi
    return capi


def _worst(family, w):
    print(f'[worst] {family}: {w:.3f} of the bound')


def _close(got, f64, f32, what, **kw):
    return R.assert_f64_close(got.detach().double().cpu().numpy() if torch.is_tensor(got) else got,
                              f64.double().cpu().numpy(), f32.double().cpu().numpy(), what=what, **kw)


# ---------------------------------------------------------------------------------------------------------------------------------------
# GRU sequence (few-column vector-ALU form up to 1024 columns, MFMA form above)
# ---------------------------------------------------------------------------------------------------------------------------------------
GSEQ_SMALL_MAX = 1024
GRU_CASES = [(1, 1), (3, 2), (4, 8), (5, 20), (147, 8), (1023, 2), (1024, 20), (1025, 1), (1029, 20), (1029, 2), (7392, 2)]


def _gru_weights(rng):
    k = 1 / np.sqrt(96)
    return (rng.uniform(-k, k, (288, 96)).astype(np.float32), rng.uniform(-k, k, 288).astype(np.float32))


def test_gru_seq_forward_and_backward_vs_float64():
    """H (H[0] written by the launch), tapes r | z | n | gh_n, hfinal (null, a padded row block, the caller's inp[:, ST:] with ld = IN),
    dgi, dgh with dh_last read through a stride -- both forms, both sides of 1024 columns, m not a multiple of 4 or 16 in each form."""
    capi, dev = _capi(), _gpu()
    st = capi.stream_ptr()
    rng = np.random.default_rng(11)
    Whh, bhh = _gru_weights(rng)
    dW, db = torch.from_numpy(Whh).to(dev), torch.from_numpy(bhh).to(dev)
    worst = {}
    forms = set()
    for ci, (m, Tp) in enumerate(GRU_CASES):
        forms.add(m <= GSEQ_SMALL_MAX)
        gi = (rng.standard_normal((m, Tp, 288)) * 1.5).astype(np.float32)
        dh = rng.standard_normal((m, 96)).astype(np.float32)
        H = torch.full((Tp + 1, m, 96), float('nan'), device=dev)
        tapes = torch.full((Tp, m, 384), float('nan'), device=dev)
        hf_kind = ci % 3                                   # 0: null, 1: rows of 100 floats, 2: the caller's inp[:, ST:] (ld = IN = 256)
        ldhf = {0: 96, 1: 100, 2: 256}[hf_kind]
        hbuf = torch.full((m, ldhf), SENT, device=dev)
        hfin = None if hf_kind == 0 else (hbuf if hf_kind == 1 else hbuf[:, 160:])
        capi.call('sttode_gru_seq_fwd', torch.from_numpy(gi).to(dev), dW, db, H, tapes, hfin, ldhf, m, Tp, st)
        # dh_last strided: a column block of a wider matrix (ld 100, or the caller's din[:, ST:] with ld 256)
        lddh = 100 if ci % 2 else 256
        dbuf = torch.full((m, lddh), float('nan'), device=dev)
        off = 0 if ci % 2 else 160
        dbuf[:, off:off + 96] = torch.from_numpy(dh).to(dev)
        dgi = torch.full((m, Tp, 288), float('nan'), device=dev)
        dgh = torch.full((Tp, m, 288), float('nan'), device=dev)
        capi.call('sttode_gru_seq_bwd', dbuf[:, off:], lddh, tapes, H, dW, dgi, dgh, m, Tp, st)
        torch.cuda.synchronize()
        args = [torch.from_numpy(a) for a in (gi, Whh, bhh, dh)]
        r64 = R.gru_seq(*[a.double() for a in args])
        r32 = R.gru_seq(*args)
        what = f'gru_seq m={m} Tp={Tp}'
        form = 'small' if m <= GSEQ_SMALL_MAX else 'mfma'
        for k in ('H', 'tapes', 'dgi', 'dgh'):
            got = {'H': H, 'tapes': tapes, 'dgi': dgi, 'dgh': dgh}[k]
            w = _close(got, r64[k], r32[k], f'{what} {k}')
            worst[(form, k)] = max(worst.get((form, k), 0.0), w)
        assert torch.equal(H[0].cpu(), torch.zeros(m, 96)), what
        if hf_kind:
            hb = hbuf.cpu()
            c0 = 0 if hf_kind == 1 else 160
            w = _close(hb[:, c0:c0 + 96], r64['H'][Tp], r32['H'][Tp], f'{what} hfinal')
            worst[(form, 'hfinal')] = max(worst.get((form, 'hfinal'), 0.0), w)
            rest = torch.cat([hb[:, :c0], hb[:, c0 + 96:]], 1)
            assert (rest == SENT).all(), f'{what}: hfinal wrote outside its 96 columns'
    assert forms == {True, False}
    for k, w in sorted(worst.items()):
        _worst(f'gru_seq {k[0]} {k[1]}', w)


def test_gru_seq_refuses_misaligned_pointers_and_writes_nothing():
    capi, dev = _capi(), _gpu()
    st = capi.stream_ptr()
    m, Tp = 8, 3
    gi = torch.zeros(m * Tp * 288 + 4, device=dev)
    W, b = torch.zeros(288, 96, device=dev), torch.zeros(288, device=dev)
    H = torch.full((Tp + 1, m, 96), SENT, device=dev)
    tapes = torch.full((Tp, m, 384), SENT, device=dev)
    hf = torch.full((m, 104), SENT, device=dev)
    for name, args in (('gi', (gi[1:], None, 96)), ('hfinal', (gi[:-4], hf[:, 1:], 100)), ('ldhf', (gi[:-4], hf, 98)),
                       ('ldhf < 96', (gi[:-4], hf, 92))):
        with pytest.raises(capi.SttodeError):
            capi.call('sttode_gru_seq_fwd', args[0], W, b, H, tapes, args[1], args[2], m, Tp, st)
    dh = torch.zeros(m, 100, device=dev)
    dgi = torch.full((m, Tp, 288), SENT, device=dev)
    dgh = torch.full((Tp, m, 288), SENT, device=dev)
    with pytest.raises(capi.SttodeError):
        capi.call('sttode_gru_seq_bwd', dh[:, 1:], 100, tapes, H, W, dgi, dgh, m, Tp, st)
    torch.cuda.synchronize()
    for t in (H, tapes, hf, dgi, dgh):
        assert (t == SENT).all()


def test_gru_cell_forward_and_backward_vs_float64():
    """sttode_gru_cell_fwd / _bwd (in the ABI, no Python caller): hprev null and given, gi rows read through a stride."""
    capi, dev = _capi(), _gpu()
    st = capi.stream_ptr()
    rng = np.random.default_rng(12)
    worst = 0.0
    for m in (1, 7, 1000):
        for with_h in (False, True):
            ldgi = 300
            gi = (rng.standard_normal((m, 288)) * 1.5).astype(np.float32)
            gh = (rng.standard_normal((m, 288)) * 0.7).astype(np.float32)
            hp = rng.standard_normal((m, 96)).astype(np.float32) if with_h else None
            dh = rng.standard_normal((m, 96)).astype(np.float32)
            gib = torch.full((m, ldgi), SENT, device=dev)
            gib[:, :288] = torch.from_numpy(gi).to(dev)
            hnew = torch.full((m, 96), float('nan'), device=dev)
            tape = torch.full((m, 384), float('nan'), device=dev)
            hpd = None if hp is None else torch.from_numpy(hp).to(dev)
            capi.call('sttode_gru_cell_fwd', gib, ldgi, torch.from_numpy(gh).to(dev), hpd, hnew, tape, m, st)
            dgi = torch.full((m, ldgi), SENT, device=dev)
            dgh = torch.full((m, 288), float('nan'), device=dev)
            dhp = torch.full((m, 96), float('nan'), device=dev)
            capi.call('sttode_gru_cell_bwd', torch.from_numpy(dh).to(dev), tape, hpd, dgi, ldgi, dgh, dhp, m, st)
            torch.cuda.synchronize()
            a = [torch.from_numpy(gi), torch.from_numpy(gh), None if hp is None else torch.from_numpy(hp), torch.from_numpy(dh)]
            r64 = R.gru_cell(*[None if x is None else x.double() for x in a])
            r32 = R.gru_cell(*a)
            what = f'gru_cell m={m} hprev={with_h}'
            for k, got in (('hnew', hnew), ('tape', tape), ('dgi', dgi[:, :288]), ('dgh', dgh), ('dhprev', dhp)):
                worst = max(worst, _close(got, r64[k], r32[k], f'{what} {k}'))
            assert (dgi[:, 288:] == SENT).all(), what
    _worst('gru_cell', worst)


# ---------------------------------------------------------------------------------------------------------------------------------------
# conv1d(2 -> 32, k = 3) + relu: forward, input gradient, weight gradient (one workgroup up to 128 rows, partials + reduce above)
# ---------------------------------------------------------------------------------------------------------------------------------------
CONV_CASES = [(1, 1, 1, False), (1, 2, 1, True), (16, 8, 1, True), (129, 1, 21, True), (250, 8, 21, False), (2048, 8, 1, True),
              (3277, 5, 21, True), (5000, 8, 1, False), (105, 8, 21, False)]      # rows = m T: 1, 2, 128, 129, 2000, 16384, 16385, 40000, 840


def _conv_inputs(rng, m, T, adiv, with_xb):
    xa = rng.standard_normal(((m + adiv - 1) // adiv, T, 2)).astype(np.float32)
    xb = (rng.standard_normal((m, T, 2)) * 0.5).astype(np.float32) if with_xb else None
    w = (rng.standard_normal((32, 2, 3)) * 0.4).astype(np.float32)
    b = (rng.standard_normal(32) * 0.3).astype(np.float32)
    return xa, xb, w, b


def _conv_G(rows):
    return min((rows + 63) // 64, 256)


def test_conv_forward_and_backward_vs_float64():
    capi, dev = _capi(), _gpu()
    st = capi.stream_ptr()
    rng = np.random.default_rng(13)
    t = lambda a: None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    worst = {}
    paths = set()
    for m, T, adiv, with_xb in CONV_CASES:
        rows = m * T
        paths.add(rows <= 128)
        xa, xb, w, b = _conv_inputs(rng, m, T, adiv, with_xb)
        x = torch.full((m, T, 2), float('nan'), device=dev)
        e = torch.full((m, T, 32), float('nan'), device=dev)
        capi.call('sttode_conv_fwd', t(xa), adiv, t(xb), t(w), t(b), x, e, m, T, st)
        de = (rng.standard_normal((m, T, 32)) * (e.cpu().numpy() > 0)).astype(np.float32)     # arrives masked by the relu
        dw0, db0 = rng.standard_normal((32, 2, 3)).astype(np.float32), rng.standard_normal(32).astype(np.float32)
        dwd, dbd = t(dw0), t(db0)
        dx = torch.full((m, T, 2), float('nan'), device=dev) if rows != 840 else None          # (dx null)
        scratch = torch.full((_conv_G(rows) * 224,), float('nan'), device=dev)
        capi.call('sttode_conv_bwd', t(de), x, t(w), dx, dwd, dbd, m, T, scratch, scratch.numel(), st)
        torch.cuda.synchronize()
        a = [torch.from_numpy(v) if v is not None else None for v in (xa, xb, w, b, de)]
        r64 = R.conv(a[0].double(), adiv, None if xb is None else a[1].double(), a[2].double(), a[3].double(), a[4].double())
        r32 = R.conv(a[0], adiv, a[1], a[2], a[3], a[4])
        what = f'conv m={m} T={T} adiv={adiv} xb={with_xb}'
        path = 'one-wg' if rows <= 128 else 'partials'
        outs = [('x', x, r64['x'], r32['x']), ('e', e, r64['e'], r32['e']),
                ('dw', dwd, r64['dw'] + torch.from_numpy(dw0).double(), r32['dw'] + torch.from_numpy(dw0)),
                ('db', dbd, r64['db'] + torch.from_numpy(db0).double(), r32['db'] + torch.from_numpy(db0))]
        if dx is not None:
            outs.append(('dx', dx, r64['dx'], r32['dx']))
        for k, got, f64, f32 in outs:
            w_ = _close(got, f64, f32, f'{what} {k}')
            worst[(path, k)] = max(worst.get((path, k), 0.0), w_)
    assert paths == {True, False}
    for k, w in sorted(worst.items()):
        _worst(f'conv {k[0]} {k[1]}', w)


def test_conv_weight_gradient_is_deterministic_and_refuses_small_scratch():
    capi, dev = _capi(), _gpu()
    st = capi.stream_ptr()
    rng = np.random.default_rng(14)
    m, T = 5000, 8
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    xa, xb, w, b = _conv_inputs(rng, m, T, 1, True)
    x, e = torch.empty((m, T, 2), device=dev), torch.empty((m, T, 32), device=dev)
    capi.call('sttode_conv_fwd', t(xa), 1, t(xb), t(w), t(b), x, e, m, T, st)
    de = t(rng.standard_normal((m, T, 32)).astype(np.float32)) * (e > 0)
    G = _conv_G(m * T)
    runs = []
    for _ in range(2):
        dwd, dbd = torch.ones(32, 2, 3, device=dev), torch.ones(32, device=dev)
        scratch = torch.empty(G * 224, device=dev)
        capi.call('sttode_conv_bwd', de, x, t(w), None, dwd, dbd, m, T, scratch, scratch.numel(), st)
        runs.append((dwd.cpu(), dbd.cpu()))
    assert torch.equal(runs[0][0], runs[1][0]) and torch.equal(runs[0][1], runs[1][1])
    # scratch one float short: refused before anything is written (dx included)
    dx = torch.full((m, T, 2), SENT, device=dev)
    dwd, dbd = torch.full((32, 2, 3), SENT, device=dev), torch.full((32,), SENT, device=dev)
    scratch = torch.full((G * 224,), SENT, device=dev)
    with pytest.raises(capi.SttodeError):
        capi.call('sttode_conv_bwd', de, x, t(w), dx, dwd, dbd, m, T, scratch, G * 224 - 1, st)
    torch.cuda.synchronize()
    for v in (dx, dwd, dbd, scratch):
        assert (v == SENT).all()


# ---------------------------------------------------------------------------------------------------------------------------------------
# LayerNorm(x + r): D = 32 / 64 / 128; backward in one workgroup up to 64 rows, partials + reduce above (G capped at 256)
# ---------------------------------------------------------------------------------------------------------------------------------------
LN_ROWS = (1, 3, 4, 5, 64, 65, 4096, 4097, 20000)


def _ln_G(rows):
    return 1 if rows <= 64 else min((rows + 15) // 16, 256)


def _ln_inputs(rng, rows, D, with_r):
    # row scales from 3e-3 to 10: small-variance rows make eps matter.  The row means stay within a few standard deviations: an offset of
    # 1 on a row of scale 3e-3 (measured: 2e-5 off in y at D = 32) is the fp32 cancellation of any one-pass mean, not a kernel error
    sc = 10.0 ** rng.uniform(-2.5, 1.0, (rows, 1))
    x = ((rng.standard_normal((rows, D)) + 2 * rng.standard_normal((rows, 1))) * sc).astype(np.float32)
    r = (rng.standard_normal((rows, D)) * sc).astype(np.float32) if with_r else None
    g = (1 + 0.3 * rng.standard_normal(D)).astype(np.float32)
    b = (0.3 * rng.standard_normal(D)).astype(np.float32)
    dy = rng.standard_normal((rows, D)).astype(np.float32)
    return x, r, g, b, dy


def test_layernorm_forward_and_backward_vs_float64():
    capi, dev = _capi(), _gpu()
    st = capi.stream_ptr()
    rng = np.random.default_rng(15)
    t = lambda a: None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    worst = {}
    for D in (32, 64, 128):
        for ri, rows in enumerate(LN_ROWS):
            with_r = (ri + D // 32) % 2 == 1
            x, r, g, b, dy = _ln_inputs(rng, rows, D, with_r)
            y = torch.full((rows, D), float('nan'), device=dev)
            xh = torch.full((rows, D), float('nan'), device=dev)
            rs = torch.full((rows,), float('nan'), device=dev)
            capi.call('sttode_add_ln_fwd', t(x), t(r), t(g), t(b), y, xh, rs, rows, D, st)
            dsum = torch.full((rows, D), float('nan'), device=dev)
            dg0, db0 = rng.standard_normal(D).astype(np.float32), rng.standard_normal(D).astype(np.float32)
            dgd, dbd = t(dg0), t(db0)
            scratch = torch.full((_ln_G(rows) * 2 * D,), float('nan'), device=dev)
            capi.call('sttode_ln_bwd', t(dy), xh, rs, t(g), dsum, dgd, dbd, rows, D, scratch, scratch.numel(), st)
            torch.cuda.synchronize()
            a = [None if v is None else torch.from_numpy(v) for v in (x, r, g, b, dy)]
            r64 = R.add_ln(*[None if v is None else v.double() for v in a])
            r32 = R.add_ln(*a)
            what = f'layernorm D={D} rows={rows} r={with_r}'
            path = 'one-wg' if rows <= 64 else 'partials'
            for k, got, f64, f32 in (('y', y, r64['y'], r32['y']), ('xhat', xh, r64['xhat'], r32['xhat']), ('rstd', rs, r64['rstd'], r32['rstd']),
                                     ('dsum', dsum, r64['dsum'], r32['dsum']),
                                     ('dgamma', dgd, r64['dgamma'] + torch.from_numpy(dg0).double(), r32['dgamma'] + torch.from_numpy(dg0)),
                                     ('dbeta', dbd, r64['dbeta'] + torch.from_numpy(db0).double(), r32['dbeta'] + torch.from_numpy(db0))):
                w_ = _close(got, f64, f32, f'{what} {k}')
                worst[(D, path, k)] = max(worst.get((D, path, k), 0.0), w_)
    for k, w in sorted(worst.items()):
        _worst(f'layernorm D={k[0]} {k[1]} {k[2]}', w)


def test_layernorm_backward_is_deterministic_and_refusals_write_nothing():
    capi, dev = _capi(), _gpu()
    st = capi.stream_ptr()
    rng = np.random.default_rng(16)
    t = lambda a: None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    rows, D = 4097, 128
    x, r, g, b, dy = _ln_inputs(rng, rows, D, True)
    y, xh, rs = torch.empty((rows, D), device=dev), torch.empty((rows, D), device=dev), torch.empty(rows, device=dev)
    capi.call('sttode_add_ln_fwd', t(x), t(r), t(g), t(b), y, xh, rs, rows, D, st)
    G = _ln_G(rows)
    runs = []
    for _ in range(2):
        dsum, dgd, dbd = torch.empty((rows, D), device=dev), torch.ones(D, device=dev), torch.ones(D, device=dev)
        scratch = torch.empty(G * 2 * D, device=dev)
        capi.call('sttode_ln_bwd', t(dy), xh, rs, t(g), dsum, dgd, dbd, rows, D, scratch, scratch.numel(), st)
        runs.append((dsum.cpu(), dgd.cpu(), dbd.cpu()))
    assert all(torch.equal(p, q) for p, q in zip(*runs))
    # scratch one float short; D = 48
    bufs = [torch.full((rows, D), SENT, device=dev) for _ in range(3)] + [torch.full((D,), SENT, device=dev) for _ in range(2)]
    scratch = torch.full((G * 2 * D,), SENT, device=dev)
    with pytest.raises(capi.SttodeError):
        capi.call('sttode_ln_bwd', t(dy), xh, rs, t(g), bufs[0], bufs[3], bufs[4], rows, D, scratch, G * 2 * D - 1, st)
    g48 = torch.ones(48, device=dev)
    with pytest.raises(capi.SttodeError):
        capi.call('sttode_add_ln_fwd', t(x), None, g48, g48, bufs[1], bufs[2], bufs[0][:, 0], rows // 2, 48, st)
    with pytest.raises(capi.SttodeError):
        capi.call('sttode_ln_bwd', t(dy), xh, rs, g48, bufs[0], bufs[3], bufs[4], rows // 2, 48, scratch, scratch.numel(), st)
    torch.cuda.synchronize()
    for v in bufs + [scratch]:
        assert (v == SENT).all()


# ---------------------------------------------------------------------------------------------------------------------------------------
# sttode_tlinear_tab: every form tlinear_impl can reach, with a per-group table as the accumulate source
# ---------------------------------------------------------------------------------------------------------------------------------------
TGEMM_MIN_COLS, TGEMM_MIN_COLS_BWD, TLIN_MEDIUM_BELOW = 2048, 600, 4096


def _tlin_form(cols, I):
    if cols > TGEMM_MIN_COLS:
        return 'lds-tiled'
    if cols <= 1024:
        return 'latency'
    return 'medium' if ((cols + 63) // 64) * ((I + 63) // 64) < TLIN_MEDIUM_BELOW else 'throughput'


# cols, J, I, tdiv, table aligned (vector epilogue where I % 4 == 0), bias, act
TAB_CASES = [(1, 33, 64, 1, True, True, 0), (17, 128, 70, 7, False, False, 1), (17, 40, 64, 7, False, True, 3), (1024, 128, 256, 21, True, True, 2),
             (1025, 64, 96, 21, False, True, 3), (1500, 100, 130, 7, True, False, 1), (1500, 96, 128, 1, True, True, 0),
             (2048, 9, 8200, 21, True, False, 0), (2049, 128, 512, 21, False, True, 1), (7392, 128, 512, 21, True, True, 1),
             (7392, 67, 130, 7, True, False, 2), (2100, 32, 64, 1, False, False, 3)]


def _tab_run(capi, dev, st, cases, inputs, grouped):
    outs = []
    if grouped:
        capi.call('sttode_tgemm_group', 1)
    try:
        for (cols, J, I, tdiv, aligned, with_b, act), (Xb, W, b, tabb) in zip(cases, inputs):
            X = Xb[:, :J]
            ldt = tabb.stride(0)
            tab = tabb[:, :I] if aligned else tabb[:, 1:I + 1]
            Y = torch.full((cols, (I + 7) // 4 * 4), SENT, device=dev)                  # 16-byte rows: the table decides the epilogue
            capi.call('sttode_tlinear_tab', X, X.stride(0), W, J, b if with_b else None, tab, ldt, tdiv, Y, Y.stride(0), cols, J, I, act, st)
            outs.append(Y)
    finally:
        if grouped:
            capi.call('sttode_tgemm_group', 0)
    torch.cuda.synchronize()
    return [y.cpu() for y in outs]


def test_tlinear_tab_every_form_vs_float64_and_grouped_is_bitwise_the_same():
    capi, dev = _capi(), _gpu()
    st = capi.stream_ptr()
    rng = np.random.default_rng(17)
    inputs, forms = [], set()
    for cols, J, I, tdiv, aligned, with_b, act in TAB_CASES:
        forms.add(_tlin_form(cols, I))
        groups = (cols + tdiv - 1) // tdiv
        Xb = torch.from_numpy(rng.standard_normal((cols, J + 3)).astype(np.float32)).to(dev)             # X a strided view (ld J + 3)
        W = torch.from_numpy((rng.standard_normal((I, J)) / np.sqrt(J)).astype(np.float32)).to(dev)
        b = torch.from_numpy((0.5 * rng.standard_normal(I)).astype(np.float32)).to(dev)
        ldt = ((I + 1 + 3) // 4) * 4 if aligned else I + 3                                                 # aligned rows: 16-byte multiples
        tabb = torch.from_numpy(rng.standard_normal((groups, ldt)).astype(np.float32)).to(dev)
        inputs.append((Xb, W, b, tabb))
    assert forms == {'latency', 'medium', 'throughput', 'lds-tiled'}, forms
    plain = _tab_run(capi, dev, st, TAB_CASES, inputs, False)
    worst = {}
    for (cols, J, I, tdiv, aligned, with_b, act), (Xb, W, b, tabb), Y in zip(TAB_CASES, inputs, plain):
        tab = (tabb[:, :I] if aligned else tabb[:, 1:I + 1]).cpu()
        a32 = [Xb[:, :J].cpu(), W.cpu(), b.cpu() if with_b else None, tab]
        f64 = R.tlinear_tab(*[None if v is None else v.double() for v in a32[:3]], a32[3].double(), tdiv, act)
        f32 = R.tlinear_tab(*a32[:3], a32[3], tdiv, act)
        key = (_tlin_form(cols, I), 'vector' if aligned and I % 4 == 0 else 'scalar')
        worst[key] = max(worst.get(key, 0.0), _close(Y[:, :I], f64, f32, f'tlinear_tab {cols}x{J}->{I} tdiv={tdiv} act={act} {key}'))
        assert (Y[:, I:] == SENT).all()
    # the same calls queued in an open sttode_tgemm_group: the same kernels' arithmetic, bitwise
    grouped = _tab_run(capi, dev, st, TAB_CASES, inputs, True)
    for c, p, q in zip(TAB_CASES, plain, grouped):
        assert torch.equal(p, q), f'tlinear_tab {c}: grouped launch differs'
    for k, w in sorted(worst.items()):
        _worst(f'tlinear_tab {k[0]} {k[1]}', w)
    # ldt < I: refused, nothing written
    Xb, W, b, tabb = inputs[0]
    Y = torch.full((1, 64), SENT, device=dev)
    with pytest.raises(capi.SttodeError):
        capi.call('sttode_tlinear_tab', Xb, Xb.stride(0), W, 33, None, tabb, 63, 1, Y, 64, 1, 33, 64, 0, st)
    torch.cuda.synchronize()
    assert (Y == SENT).all()


# ---------------------------------------------------------------------------------------------------------------------------------------
# sttode_train_ewise: every op code against the float64 restatement of the enum's comments
# ---------------------------------------------------------------------------------------------------------------------------------------
def _ew_cases(rng):
    """-> list of (label, op, [p0..p4 as float32 arrays or None], count, i0, f0)."""
    O = R.EW_OPS
    N = 1283                                           # not a multiple of 256
    f = lambda *s: rng.standard_normal(s).astype(np.float32).ravel()
    tanh = lambda n: np.tanh(2 * rng.standard_normal(n)).astype(np.float32)
    sig = lambda n: (1 / (1 + np.exp(-2 * rng.standard_normal(n)))).astype(np.float32)
    pad = lambda a: np.concatenate([a, np.full(5, SENT, np.float32)])    # output tails that must stay untouched
    cs = [('mul', O['MUL'], [pad(f(N)), f(N), f(N), None, None], N, 0, 0.0),
          ('axpy', O['AXPY'], [pad(f(N)), f(N), None, None, None], N, 0, -0.7),
          ('gate_bwd', O['GATE_BWD'], [f(N), tanh(N), sig(N), pad(f(N)), pad(f(N))], N, 0, 0.0),
          ('euler_fwd', O['EULER_FWD'], [pad(f(N)), f(N), f(N), None, None], N, 0, 0.37),
          ('euler_bwd', O['EULER_BWD'], [f(N), f(N), None, pad(f(N)), pad(f(N))], N, 0, 0.37)]
    rows, zd = 107, 12                                 # rsample: params [rows, 2 zd] (mu | logvar), eps [rows, zd]
    prm = np.concatenate([f(rows, zd).reshape(rows, zd), (0.8 * f(rows, zd)).reshape(rows, zd)], 1).ravel()
    cs += [('rsample', O['RSAMPLE'], [pad(f(rows * zd)), prm, f(rows * zd), None, None], rows * zd, zd, 0.0),
           ('rsample_bwd', O['RSAMPLE_BWD'], [f(rows * zd), prm, f(rows * zd), pad(f(rows * 2 * zd)), None], rows * zd, zd, 0.0),
           ('relu_bwd', O['RELU_BWD'], [pad(f(N)), f(N), f(N), None, None], N, 0, 0.0),
           ('fill', O['FILL'], [pad(f(N)), None, None, None, None], N, 0, 2.5)]
    n, K, L = 13, 7, 6                                 # cur_add / sum_cur: rows c = (agent c / K), row length L, p1 / p3 [n, 2]
    cs += [('cur_add', O['CUR_ADD'], [pad(f(n * K * L)), f(n * 2), None, None, None], n * K * L, L, float(K)),
           ('sum_cur', O['SUM_CUR'], [pad(f(n * K * L)), f(n * K * L), f(n * K * L), f(n * 2), None], n * K * L, L, float(K)),
           ('sum_cur p3 null', O['SUM_CUR'], [pad(f(n * K * L)), f(n * K * L), f(n * K * L), None, None], n * K * L, L, float(K)),
           ('tanh_bwd', O['TANH_BWD'], [pad(f(N)), f(N), tanh(N), None, None], N, 0, 0.0)]
    n, K, nz = 9, 20, 8                                # latent_bwd: A viewed [n, K nz]; eps [nz] (shared) or [n, nz] (per agent)
    cnt = n * K * nz
    A = (np.sign(f(cnt)) * (0.05 + np.abs(f(cnt)))).astype(np.float32)
    for mode, e in ((0, None), (1, f(nz)), (2, f(n * nz))):
        cs.append((f'latent_bwd mode {mode}', O['LATENT_BWD'], [f(cnt), f(cnt), A, e if e is not None else f(4), pad(f(cnt))], cnt,
                   (nz << 2) | mode, float(K * nz)))
    rows = 37
    for D in (0, 32, 64, 128):                         # euler_bwd_cat: rows of p0 = cat(dx0 | dode) with leading dimension ld; D = 0 means 64
        Dv = D or 64
        ld = 2 * Dv + 3
        cs.append((f'euler_bwd_cat D={D}', O['EULER_BWD_CAT'], [f(rows * ld), f(rows * Dv), None, pad(f(rows * Dv)), pad(f(rows * Dv))],
                   rows * Dv, ld | (D << 16), 0.61))
    cs += [('scale_add', O['SCALE_ADD'], [pad(f(N)), f(N), None, None, None], N, 0, 0.9),
           ('scale_add p1 null', O['SCALE_ADD'], [pad(f(N)), None, None, None, None], N, 0, 0.9)]
    rows, width, ld = 41, 37, 50                       # axpy_rows: a column block (width) of a wider matrix (ld)
    cs.append(('axpy_rows', O['AXPY_ROWS'], [pad(f(rows * width)), f(rows * ld), None, None, None], rows * width, width | (ld << 16), -1.3))
    return cs


def _ew_launch(capi, dev, st, case):
    label, op, p, count, i0, f0 = case
    d = [None if a is None else torch.from_numpy(a.copy()).to(dev) for a in p]
    capi.call('sttode_train_ewise', op, d[0], d[1], d[2], d[3], d[4], count, i0, f0, st)
    return d


def test_train_ewise_every_op_vs_float64():
    capi, dev = _capi(), _gpu()
    st = capi.stream_ptr()
    cases = _ew_cases(np.random.default_rng(18))
    assert {c[1] for c in cases} == set(range(16))
    results = [_ew_launch(capi, dev, st, c) for c in cases]
    torch.cuda.synchronize()
    worst = 0.0
    for (label, op, p, count, i0, f0), d in zip(cases, results):
        ref = R.ewise(op, p, count, i0, float(np.float32(f0)))
        for k, (val, scale) in ref.items():
            got = d[k].cpu().numpy().astype(np.float64)
            err, bound = np.abs(got - val), R.ulps_f32(scale, 4)
            bad = ~(err <= bound)
            assert not bad.any(), (f'ewise {label} p{k}: {int(bad.sum())} / {bad.size} out of 4 ulps of the largest term; first at '
                                   f'{int(np.argmax(bad))}: got {got[np.argmax(bad)]:.9g}, f64 {val[np.argmax(bad)]:.9g}')
            worst = max(worst, float((err / np.maximum(bound, 1e-300)).max()))
        for k, a in enumerate(p):                  # inputs are not written
            if k not in ref and a is not None:
                assert np.array_equal(d[k].cpu().numpy(), a), f'ewise {label}: input p{k} changed'
    _worst('ewise (units of 4 ulps of the largest term)', worst)


def test_train_ewise_grouped_is_bitwise_the_same_and_bad_op_is_refused():
    """Five pieces queued in an open group (the fifth launches the first four) equal the single launches bit for bit."""
    capi, dev = _capi(), _gpu()
    st = capi.stream_ptr()
    cases = _ew_cases(np.random.default_rng(19))
    pick = [c for c in cases if c[0] in ('mul', 'gate_bwd', 'rsample_bwd', 'latent_bwd mode 2', 'euler_bwd_cat D=0', 'axpy_rows')]
    single = [_ew_launch(capi, dev, st, c) for c in pick]
    capi.call('sttode_tgemm_group', 1)
    try:
        grouped = [_ew_launch(capi, dev, st, c) for c in pick]
    finally:
        capi.call('sttode_tgemm_group', 0)
    torch.cuda.synchronize()
    for c, s, g in zip(pick, single, grouped):
        for k in range(5):
            if s[k] is not None:
                assert torch.equal(s[k], g[k]), f'ewise {c[0]} p{k}: grouped launch differs'
    buf = torch.full((300,), SENT, device=dev)
    for op in (-1, 16):
        with pytest.raises(capi.SttodeError):
            capi.call('sttode_train_ewise', op, buf, buf, buf, buf, buf, 300, 0, 1.0, st)
    torch.cuda.synchronize()
    assert (buf == SENT).all()


# ---------------------------------------------------------------------------------------------------------------------------------------
# group mode across its queues (LDS-tiled products, scene-size products, element-wise pieces, deferred split sums) and its error paths
# ---------------------------------------------------------------------------------------------------------------------------------------
GROUP_MULTI_MAX = 4                      # TG_MULTI_MAX == TS_MULTI_MAX == EW_MULTI_MAX
BIG = (TGEMM_MIN_COLS + 1, 16, 16)       # cols, J, I: the first column count on the LDS-tiled forward kernel
SMALL = (17, 33, 20)                     # a scene-size product (latency mode)
RS_ROWS, RS_ZD = 8, 12                   # the reparameterisation (op 5): count 96
BWD = (TGEMM_MIN_COLS_BWD + 1, 8, 8)     # cols, N, K: the first column count whose backward products are LDS-tiled (split sums: S = 5)


def _group_inputs(dev, rng, reps):
    t = lambda *s: torch.from_numpy(rng.standard_normal(s).astype(np.float32)).to(dev)
    cols, N, K = BWD
    return dict(big=[(t(BIG[0], BIG[1]), t(BIG[2], BIG[1]), t(BIG[2])) for _ in range(reps)],
                small=[(t(SMALL[0], SMALL[1]), t(SMALL[2], SMALL[1]), t(SMALL[2])) for _ in range(reps)],
                ew=[(t(RS_ROWS, 2 * RS_ZD), t(RS_ROWS, RS_ZD)) for _ in range(reps)],
                bwd=(t(cols, N), t(N, K), t(cols, K)))


def _sent(dev, rows, width):
    """A sentinel-filled output of `width` logical columns in rows of width + 4 floats."""
    return torch.full((rows, width + 4), SENT, device=dev)


def _group_issue(capi, dev, st, inp, with_bwd=True):
    """Issues the calls of ``inp`` in turn (one of each kind, then the next of each) and returns {label: (output buffer, logical width)}."""
    outs = {}
    for i, ((Xb, Wb, bb), (Xs, Ws, bs), (prm, eps)) in enumerate(zip(inp['big'], inp['small'], inp['ew'])):
        for tag, (cols, J, I), X, W, b in (('big', BIG, Xb, Wb, bb), ('small', SMALL, Xs, Ws, bs)):
            Y = _sent(dev, cols, I)
            capi.call('sttode_tlinear', X, J, 1, W, J, 0, b, None, 0, Y, Y.stride(0), cols, J, I, 2, 0, st)
            outs[f'{tag} {i}'] = (Y, I)
        z = _sent(dev, 1, RS_ROWS * RS_ZD)
        capi.call('sttode_train_ewise', R.EW_OPS['RSAMPLE'], z, prm, eps, None, None, RS_ROWS * RS_ZD, RS_ZD, 0.0, st)
        outs[f'ew {i}'] = (z, RS_ROWS * RS_ZD)
    if with_bwd:
        cols, N, K = BWD
        dY, W, X = inp['bwd']
        dX, dW, db = _sent(dev, cols, K), _sent(dev, N, K), _sent(dev, 1, N)
        scratch = torch.zeros(64 * N * (K + 1), device=dev)
        capi.call('sttode_tlinear_bwd', dY, N, W, K, None, 0, dX, dX.stride(0), K, 0, X, K, 1, dW, dW.stride(0), db, cols, N, K,
                  scratch, scratch.numel(), st)
        outs.update({'bwd dX': (dX, K), 'bwd dW': (dW, K), 'bwd db': (db, N)})
        outs['_scratch'] = (scratch, scratch.numel())          # (kept alive until the launches have run)
    return outs


def test_one_group_across_every_queue_is_bitwise_the_ungrouped_calls():
    """Five LDS-tiled forward products, five scene-size products, five element-wise pieces (one more than each queue holds: every queue
    takes its overflow flush) and one LDS-tiled layer backward (a weight gradient with split sums) in ONE group on one stream: every
    output equals the same call made outside a group bit for bit, and nothing beyond an output's logical width is written."""
    capi, dev = _capi(), _gpu()
    st = capi.stream_ptr()
    inp = _group_inputs(dev, np.random.default_rng(23), GROUP_MULTI_MAX + 1)
    plain = _group_issue(capi, dev, st, inp)
    torch.cuda.synchronize()
    capi.call('sttode_tgemm_group', 1)
    try:
        grouped = _group_issue(capi, dev, st, inp)
    finally:
        capi.call('sttode_tgemm_group', 0)
    torch.cuda.synchronize()
    assert len(plain) == 3 * (GROUP_MULTI_MAX + 1) + 4
    for label, (p, width) in plain.items():
        if label.startswith('_'):
            continue
        g = grouped[label][0]
        assert not (p[:, :width] == SENT).any(), f'{label}: the ungrouped call left part of its output unwritten'
        assert torch.equal(p[:, :width], g[:, :width]), f'{label}: the grouped call differs from the ungrouped one'
        assert (p[:, width:] == SENT).all() and (g[:, width:] == SENT).all(), f'{label}: written beyond its logical width'


def test_group_and_deferred_reduction_error_paths_forget_what_is_queued():
    """sttode_tgemm_group(-1): whatever the open group has queued, in each of its queues, is never launched, and the group is closed.
    sttode_twgrad_defer(-1, ..): a split weight gradient whose reduction was deferred has written its partial sums to the deferral buffer;
    the pending reduction is forgotten, so dW and db stay untouched (observed on the library before and after the kernels moved to one
    file per family).  The next sttode_twgrad, without deferral, runs its own reduction and gives the float64 gradient."""
    capi, dev = _capi(), _gpu()
    st = capi.stream_ptr()
    rng = np.random.default_rng(24)
    inp = _group_inputs(dev, rng, 1)
    try:
        capi.call('sttode_tgemm_group', 1)
        queued = _group_issue(capi, dev, st, inp, with_bwd=False)
        capi.call('sttode_tgemm_group', -1)
        torch.cuda.synchronize()
        assert len(queued) == 3
        for label, (y, _) in queued.items():
            assert (y == SENT).all(), f'{label}: launched although the group was abandoned'
        (cols, J, I), (X, W, b) = SMALL, inp['small'][0]
        Y = _sent(dev, cols, I)
        capi.call('sttode_tlinear', X, J, 1, W, J, 0, b, None, 0, Y, Y.stride(0), cols, J, I, 2, 0, st)   # no group call in between
        torch.cuda.synchronize()
        assert not (Y[:, :I] == SENT).any(), 'a call after sttode_tgemm_group(-1) was queued: the group is still open'
        assert (Y[:, I:] == SENT).all()
        a32 = [X.cpu(), W.cpu(), b.cpu(), torch.zeros(cols, I)]
        _close(Y[:, :I], R.tlinear_tab(*[v.double() for v in a32], 1, 2), R.tlinear_tab(*a32, 1, 2), 'tlinear after an abandoned group')

        cols, N, K = BWD
        dY, _, X = inp['bwd']
        buf, scratch = torch.zeros(4096, device=dev), torch.zeros(64 * N * (K + 1), device=dev)
        dW, db = _sent(dev, N, K), _sent(dev, 1, N)
        capi.call('sttode_twgrad_defer', 1, buf, buf.numel())
        capi.call('sttode_twgrad', dY, N, X, K, 1, dW, dW.stride(0), db, cols, N, K, scratch, scratch.numel(), st)
        capi.call('sttode_twgrad_defer', -1, None, 0)
        torch.cuda.synchronize()
        assert (buf != 0).any() and (scratch == 0).all(), 'the split sums of a deferred gradient go to the deferral buffer'
        assert (dW == SENT).all() and (db == SENT).all(), 'the forgotten reduction ran'
        dW, db = torch.zeros(N, K + 4, device=dev), torch.zeros(1, N + 4, device=dev)
        capi.call('sttode_twgrad', dY, N, X, K, 1, dW, dW.stride(0), db, cols, N, K, scratch, scratch.numel(), st)
        torch.cuda.synchronize()
        assert (dW[:, K:] == 0).all() and (db[:, N:] == 0).all()
        dYc, Xc = dY.cpu(), X.cpu()
        w = max(_close(dW[:, :K], dYc.double().T @ Xc.double(), dYc.T @ Xc, 'twgrad dW after a forgotten reduction'),
                _close(db[0, :N], dYc.double().sum(0), dYc.sum(0), 'twgrad db after a forgotten reduction'))
        _worst('twgrad after the error paths', w)
    finally:                                                   # (a failure above must not leave its queue to the next test's group)
        capi.call('sttode_tgemm_group', -1)
        capi.call('sttode_twgrad_defer', -1, None, 0)


def test_an_open_group_belongs_to_the_host_thread_that_opened_it():
    """The queues of a group are per host thread and nothing locks them: while the main thread's group is open with one scene-size product
    queued, the same product and an element-wise fill issued by ANOTHER thread run at once on that thread's current stream -- they are not
    queued behind the main thread's group, do not launch what it queued and do not wait for it.  Closing the group then runs the queued
    product, bit for bit the other thread's."""
    import threading
    capi, dev = _capi(), _gpu()
    rng = np.random.default_rng(25)
    cols, J, I, n_fill = 37, 67, 64, 1283
    Xb = torch.from_numpy(rng.standard_normal((cols, J + 3)).astype(np.float32)).to(dev)
    X = Xb[:, :J]                                                                                  # a strided view (ld J + 3)
    W = torch.from_numpy((rng.standard_normal((I, J)) / np.sqrt(J)).astype(np.float32)).to(dev)
    b = torch.from_numpy((0.5 * rng.standard_normal(I)).astype(np.float32)).to(dev)
    Y1, Y2 = _sent(dev, cols, I), _sent(dev, cols, I)
    fill = torch.full((n_fill + 5,), SENT, device=dev)
    tlinear = lambda Y: capi.call('sttode_tlinear', X, X.stride(0), 1, W, J, 0, b, None, 0, Y, Y.stride(0), cols, J, I, 2, 0, capi.stream_ptr())
    failed = []

    def other():
        try:
            tlinear(Y2)
            capi.call('sttode_train_ewise', R.EW_OPS['FILL'], fill, None, None, None, None, n_fill, 0, 2.5, capi.stream_ptr())
            torch.cuda.synchronize()
        except BaseException as e:                         # (reported by the main thread)
            failed.append(e)

    capi.call('sttode_tgemm_group', 1)
    try:
        tlinear(Y1)                                        # queued
        th = threading.Thread(target=other)
        th.start()
        th.join()
        assert not failed, failed
        a32 = [X.cpu(), W.cpu(), b.cpu(), torch.zeros(cols, I)]
        _worst('tlinear from a second host thread', _close(Y2[:, :I], R.tlinear_tab(*[v.double() for v in a32], 1, 2), R.tlinear_tab(*a32, 1, 2),
                                                           'tlinear from a thread without a group'))
        assert (Y2[:, I:] == SENT).all()
        assert (fill[:n_fill] == 2.5).all() and (fill[n_fill:] == SENT).all(), 'the other thread\'s fill was queued, or wrote past its count'
        assert (Y1 == SENT).all(), 'the other thread launched (or the open group did not queue) the main thread\'s product'
    finally:
        capi.call('sttode_tgemm_group', 0)
        torch.cuda.synchronize()
    assert torch.equal(Y1, Y2)


# ---------------------------------------------------------------------------------------------------------------------------------------
# row shuffles: bitwise
# ---------------------------------------------------------------------------------------------------------------------------------------
def test_rows_copy_reduce_and_decoder_inputs_are_bitwise_numpy():
    capi, dev = _capi(), _gpu()
    st = capi.stream_ptr()
    rng = np.random.default_rng(20)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    # rows_copy: dst[r, f] = src[(r / div) % mod, f], into a column block of a wider matrix
    for rows, width, div, mod, ldd, lds in ((1, 1, 1, 1, 3, 1), (133, 96, 21, 7, 256, 100), (420, 37, 1, 420, 40, 37), (300, 5, 4, 3, 9, 6)):
        src = rng.standard_normal((max(mod, 1), lds)).astype(np.float32)
        dst = torch.full((rows, ldd), SENT, device=dev)
        capi.call('sttode_rows_copy', dst, ldd, t(src), lds, rows, width, div, mod, st)
        ref = np.full((rows, ldd), SENT, np.float32)
        ref[:, :width] = src[(np.arange(rows) // div) % mod, :width]
        assert np.array_equal(dst.cpu().numpy(), ref), (rows, width, div, mod)
    # rows_reduce: dst[a, f] (+)= sum_k src[a K + k, f], k in order in fp32
    for rows_out, width, K, ldd, lds, acc in ((1, 1, 1, 1, 1, 0), (33, 96, 21, 100, 256, 0), (33, 96, 21, 100, 256, 1), (50, 128, 20, 128, 160, 1),
                                              (7, 13, 3, 13, 13, 0)):
        src = rng.standard_normal((rows_out * K, lds)).astype(np.float32)
        d0 = rng.standard_normal((rows_out, ldd)).astype(np.float32)
        dst = t(d0)
        capi.call('sttode_rows_reduce', dst, ldd, t(src), lds, rows_out, width, K, acc, st)
        s = np.zeros((rows_out, width), np.float32)
        for k in range(K):
            s = (s + src[k::K, :width]).astype(np.float32)
        ref = d0.copy()
        ref[:, :width] = (d0[:, :width] + s).astype(np.float32) if acc else s
        assert np.array_equal(dst.cpu().numpy(), ref), (rows_out, width, K, acc)
    # decoder_inputs: row c = (agent c / K1, sample c % K1) gets cat(pf[a] [pfw], z) with z = qz[a] for sample 0, eps[a, k - 1] otherwise
    for n, K1, pfw, zd, ld, two in ((1, 1, 128, 32, 260, False), (7, 21, 128, 32, 256, True), (5, 1, 64, 16, 100, True), (3, 4, 0, 8, 12, False)):
        ldpf = pfw + 4
        pf = rng.standard_normal((n, ldpf)).astype(np.float32)
        qz = rng.standard_normal((n, zd)).astype(np.float32)
        eps = rng.standard_normal((n * max(K1 - 1, 1), zd)).astype(np.float32)
        i0 = torch.full((n * K1, ld), SENT, device=dev)
        i1 = torch.full((n * K1, ld), SENT, device=dev) if two else None
        capi.call('sttode_decoder_inputs', i0, i1, ld, t(pf), ldpf, t(qz), t(eps), n, K1, pfw, zd, st)
        ref = np.full((n * K1, ld), SENT, np.float32)
        a, k = np.arange(n * K1) // K1, np.arange(n * K1) % K1
        ref[:, :pfw] = pf[a, :pfw]
        z = eps[np.maximum(a * (K1 - 1) + k - 1, 0)]
        z[k == 0] = qz[a[k == 0]]
        ref[:, pfw:pfw + zd] = z
        assert np.array_equal(i0.cpu().numpy(), ref), (n, K1, pfw, zd)
        if two:
            assert np.array_equal(i1.cpu().numpy(), ref), (n, K1, pfw, zd)


# ---------------------------------------------------------------------------------------------------------------------------------------
# Adam drop-in against torch.optim.Adam
# ---------------------------------------------------------------------------------------------------------------------------------------
def _adam_compare(oa, ob, ps_a, ps_b):
    sda, sdb = oa.state_dict(), ob.state_dict()
    for i, (pa, pb) in enumerate(zip(ps_a, ps_b)):
        torch.testing.assert_close(pa.detach(), pb.detach(), rtol=2e-6, atol=2e-7)
        for k in ('exp_avg', 'exp_avg_sq'):
            torch.testing.assert_close(oa.state[pa][k], ob.state[pb][k], rtol=2e-6, atol=1e-7)
        assert float(sda['state'][i]['step']) == float(sdb['state'][i]['step']), (i, float(sda['state'][i]['step']), float(sdb['state'][i]['step']))


def test_adam_updates_a_parameter_that_gets_its_first_gradient_later():
    """(a) Step 1 has a gradient on p0 only; steps 2-4 on both: p1 must be updated from step 2 on, as torch does."""
    from sttode_amd.optim import Adam
    dev = _gpu()
    torch.manual_seed(31)
    ps_a = [torch.nn.Parameter(torch.randn(37, device=dev)), torch.nn.Parameter(torch.randn(5, 3, device=dev))]
    ps_b = [torch.nn.Parameter(p.detach().clone()) for p in ps_a]
    oa, ob = Adam(ps_a, lr=1e-2), torch.optim.Adam(ps_b, lr=1e-2, foreach=False)
    for it in range(4):
        for j, (pa, pb) in enumerate(zip(ps_a, ps_b)):
            if it == 0 and j == 1:
                pa.grad = pb.grad = None
                continue
            g = torch.randn(pa.shape, device=dev)
            pa.grad, pb.grad = g, g.clone()
        oa.step()
        ob.step()
    _adam_compare(oa, ob, ps_a, ps_b)


def test_adam_step_count_survives_a_fallback_step():
    """(b) HIP, HIP, torch fallback (a non-contiguous gradient), HIP, HIP: the bias correction after the fallback and state_dict()'s step."""
    from sttode_amd.optim import Adam
    dev = _gpu()
    torch.manual_seed(32)
    ps_a = [torch.nn.Parameter(torch.randn(6, 6, device=dev)), torch.nn.Parameter(torch.randn(11, device=dev))]
    ps_b = [torch.nn.Parameter(p.detach().clone()) for p in ps_a]
    oa, ob = Adam(ps_a, lr=1e-2), torch.optim.Adam(ps_b, lr=1e-2, foreach=False)
    for it in range(5):
        for pa, pb in zip(ps_a, ps_b):
            g = torch.randn(pa.shape, device=dev)
            if it == 2 and pa.dim() == 2:
                g = g.t()                                  # non-contiguous: torch's own step
            pa.grad, pb.grad = g, g.clone()
        oa.step()
        ob.step()
    _adam_compare(oa, ob, ps_a, ps_b)


@pytest.mark.parametrize('amsgrad', [False, True])
def test_adam_step_returns_the_closure_loss(amsgrad):
    """(c) step(closure) returns the closure's loss on the HIP path and on the fallback (amsgrad: torch's own step)."""
    from sttode_amd.optim import Adam
    dev = _gpu()
    p = torch.nn.Parameter(torch.randn(10, device=dev))
    o = Adam([p], lr=1e-2, amsgrad=amsgrad)

    def closure():
        o.zero_grad()
        loss = (p * p).sum()
        loss.backward()
        return loss

    for _ in range(2):
        loss = o.step(closure)
        assert loss is not None and torch.is_tensor(loss) and loss.shape == ()
