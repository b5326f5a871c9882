"""-m gpu: the per-image pseudo-label refresh on the device (aide_amd/csrc/labelbank.hip,aide_amd/labelbank.py
ImageLabelBank).  The device bank reproduces fixture g24 (the reference's own statements, tools/gen_golden_image_refresh.py) and
the numpy bank byte for byte, the fused epilogue's labels are `label_map`'s, ranking and write flags follow the documented rule
for K up to 70001, `refresh` equals per-image prediction + the host rule, and the kidney / breast loops run with the switch set
and are unchanged with it off.  Integer and index results are exact; nothing here has a floating tolerance."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, 'tests', 'golden', 'g24_image_refresh.npz')


@pytest.mark.parametrize('key', ['breast12', 'kidney12', 'breast3', 'kidney3'])
def test_device_bank_against_g24(dev, key):
    sys.path.insert(0, os.path.join(ROOT, 'tests'))
    from test_image_refresh_host import follow_fixture
    g = np.load(GOLD)
    bank = follow_fixture(g, key, device=dev)
    host = follow_fixture(g, key)
    assert np.array_equal(bank.rank.cpu().numpy(), host.rank) and np.array_equal(bank.written.cpu().numpy(), host.written)
    assert np.array_equal(bank.modified.cpu().numpy(), host.modified)


def _random_case(rng, K, h, w):
    orig = ((rng.rand(K, h, w) < 0.4) * rng.randint(1, 256, (K, h, w))).astype(np.uint8)
    orig[0] = 0                                            # empty target
    if K > 3:
        orig[3] = 200                                      # constant (kidney: gate closed)
    labs = [(rng.rand(K, h, w) < 0.45).astype(np.int64) for _ in range(4)]
    for lab in labs:
        lab[0] = 0                                         # ... and empty predictions: 0.0, not written
        if K > 2:
            lab[2] = 0                                     # empty prediction, non-empty target
    return orig, labs


@pytest.mark.parametrize('form', ['breast', 'kidney'])
@pytest.mark.parametrize('shape', [(16, 16), (5, 7), (1, 1)])
def test_device_equals_host_on_random_inputs(dev, form, shape):
    """two refreshes (the second scores against what the first wrote), int64 then uint8 label maps, targets in between"""
    from aide_amd.labelbank import ImageLabelBank
    h, w = shape
    K = 37
    rng = np.random.RandomState(h * 100 + w)
    orig, labs = _random_case(rng, K, h, w)
    d = ImageLabelBank(torch.from_numpy(orig).to(dev), labelled=[1, 5], form=form, update_percent=0.4)
    c = ImageLabelBank(orig, labelled=[1, 5], form=form, update_percent=0.4)
    for e, (a, b) in enumerate(((labs[0], labs[1]), (labs[2].astype(np.uint8), labs[3].astype(np.uint8)))):
        assert d.refresh_from_labels(torch.from_numpy(a).to(dev), torch.from_numpy(b).to(dev), e, 5, batch_size=16)
        c.refresh_from_labels(a, b, e, 5)
        assert np.array_equal(d._sums.cpu().numpy(), c._sums)
        assert np.array_equal(d.image_dice().numpy().view(np.uint32), c.image_dice().numpy().view(np.uint32))
        assert np.array_equal(d.rank.cpu().numpy(), c.rank) and np.array_equal(d.written.cpu().numpy(), c.written)
        assert np.array_equal(d.bank.cpu().numpy(), c.bank) and np.array_equal(d.modified.cpu().numpy(), c.modified)
        idx = rng.randint(-2, K + 2, 50)
        for n in (1, 2):
            assert np.array_equal(d.targets(idx, n).cpu().numpy(), c.targets(idx, n).numpy())
    assert c.written.sum() > 0 and not np.array_equal(c.bank[0], orig)


def _logits(rng, n, h, w):
    """fp32 logits with planted equal pairs, pairs one ulp apart, pairs closer than the softmax resolves, NaN and infinities"""
    z = rng.randn(n, 2, h, w).astype(np.float32)
    flat = z.reshape(n, 2, -1)
    hw = h * w
    for i in range(n):
        p = rng.permutation(hw)
        q = max(1, hw // 8)
        a = p[:q]
        flat[i, 1, a] = flat[i, 0, a]                                                  # equal: label 0
        b = p[q:2 * q]
        flat[i, 1, b] = np.nextafter(flat[i, 0, b], np.float32(np.inf))                # one ulp above
        c = p[2 * q:3 * q]
        flat[i, 0, c] = 8.0
        flat[i, 1, c] = np.float32(8.0) + np.float32(2.0 ** -20)                       # above, but exp(z0 - z1) rounds to 1?
        if hw >= 8:
            flat[i, 1, p[3 * q]] = np.nan
            flat[i, 0, p[3 * q + 1]] = np.nan
            flat[i, :, p[3 * q + 2]] = np.inf
            flat[i, 0, p[3 * q + 3]] = -np.inf
    return z


@pytest.mark.parametrize('shape', [(16, 16), (5, 7), (1, 1), (72, 64)])
def test_fused_epilogue_labels_and_sums(dev, shape):
    """labels == label_map(logits) bit for bit, sums == int64 numpy; aligned (16-byte path) and misaligned `pred` views"""
    from aide_amd.inference import label_map, image_eval_logits
    h, w = shape
    K, N, k0 = 11, 5, 4
    rng = np.random.RandomState(h + w)
    z = torch.from_numpy(_logits(rng, N, h, w)).to(dev)
    want = label_map(z).cpu().numpy()
    assert 0 < want.sum() < want.size or h * w == 1
    score = ((rng.rand(N, h, w) < 0.5) * rng.randint(1, 256, (N, h, w))).astype(np.uint8)
    gate = (rng.rand(K) < 0.7).astype(np.uint8)
    gate[k0] = 0
    for use_gate in (False, True):
        for off in (0, 1):                                  # off = 1: a pred buffer one byte off any 16-byte boundary
            raw = torch.full((K * h * w + 16,), 7, device=dev, dtype=torch.uint8)
            pred = raw[off:off + K * h * w].view(K, h, w)
            sums = torch.full((K, 4), -5, device=dev, dtype=torch.int64)
            image_eval_logits(z, torch.from_numpy(score).to(dev), torch.from_numpy(gate).to(dev) if use_gate else None, k0, pred, sums)
            got = pred.cpu().numpy()
            assert np.array_equal(got[k0:k0 + N], want.astype(np.uint8))
            assert (got[:k0] == 7).all() and (got[k0 + N:] == 7).all() and (raw[off + K * h * w:] == 7).all() and (raw[:off] == 7).all()
            t = (score > 0).astype(np.int64)
            if use_gate:
                t = t * gate[k0:k0 + N, None, None].astype(np.int64)
            ref = np.stack([np.full(N, h * w), (want * t).sum((1, 2)), want.sum((1, 2)), t.sum((1, 2))], axis=1)
            s = sums.cpu().numpy()
            assert np.array_equal(s[k0:k0 + N], ref) and (s[:k0] == -5).all() and (s[k0 + N:] == -5).all()


def _rank_case(K):
    """sums [K,4] at HW = 16 built directly: half of the images at 0.0 (empty predictions, empty targets, misses), few distinct
    values elsewhere (many exact ties), n_select inside a run of equal values"""
    rng = np.random.RandomState(K)
    sums = np.zeros((K, 4), np.int64)
    sums[:, 0] = 16
    sp = rng.randint(1, 9, K)
    st = rng.randint(1, 9, K)
    spt = np.minimum(np.minimum(sp, st), rng.randint(1, 4, K))
    kind = rng.randint(0, 6, K)
    sp[kind == 0] = 0
    st[kind == 0] = 0                                       # union 0
    sp[kind == 1] = 0                                       # empty prediction
    spt[kind <= 2] = 0                                      # kind 2: a miss
    sums[:, 1], sums[:, 2], sums[:, 3] = spt, sp, st
    labelled = (rng.rand(K) < 0.1).astype(np.uint8)
    return sums, labelled


@pytest.mark.parametrize('K', [1, 255, 256, 257, 4096, 4097, 70001])
def test_ranking_and_write_flags(dev, K):
    from aide_amd.inference import image_refresh_select, image_dice_rule
    sums, labelled = _rank_case(K)
    dsums, dlab = torch.from_numpy(sums).to(dev), torch.from_numpy(labelled).to(dev)
    uni = (sums[:, 2] + sums[:, 3]).astype(np.float64)
    with np.errstate(invalid='ignore', divide='ignore'):
        want = np.where(uni == 0, 0.0, (2 * sums[:, 1]).astype(np.float64) / uni).astype(np.float32)
    order = np.lexsort((np.arange(K), want))
    ref_rank = np.empty(K, np.int64)
    ref_rank[order] = np.arange(K)
    srt = want[order]
    zeros = int((srt == 0.0).sum())
    # n_select: nothing, inside the run of zeros, at its end, inside a run of equal non-zero values, everything
    tied = [i for i in range(zeros + 1, K) if srt[i - 1] == srt[i]]
    picks = set([0, zeros // 2, zeros, K] + tied[len(tied) // 2:len(tied) // 2 + 1])
    if K >= 255:
        assert zeros > K // 3 and srt[zeros // 2 - 1] == srt[zeros // 2] == 0.0 and tied          # ties straddle n_select
    for n_select in sorted(picks):
        dice, rank, written = (t.cpu().numpy() for t in image_refresh_select(dsums, dlab, n_select))
        assert np.array_equal(dice.view(np.uint32), want.view(np.uint32))
        assert np.array_equal(rank, ref_rank)
        assert np.array_equal(written, ((ref_rank < n_select) & (sums[:, 2] > 0) & (labelled == 0)).astype(np.uint8))
        d2, r2, w2 = image_dice_rule(sums, labelled, n_select)
        assert np.array_equal(r2, rank) and np.array_equal(w2, written) and np.array_equal(d2.view(np.uint32), dice.view(np.uint32))
    _, _, w = image_refresh_select(dsums, None, K)
    assert np.array_equal(w.cpu().numpy(), (sums[:, 2] > 0).astype(np.uint8))


@pytest.mark.parametrize('K,shape', [(70001, (1, 16)), (300, (5, 7)), (9, (72, 64))])
def test_update_changes_exactly_the_written_rows(dev, K, shape):
    from aide_amd.inference import image_bank_update
    h, w = shape
    rng = np.random.RandomState(K)
    pred = (rng.rand(K, h, w) < 0.5).astype(np.uint8)
    written = (rng.rand(K) < 0.3).astype(np.uint8)
    written[[0, K - 1]] = 1
    written[K // 2] = 0
    for scale in (255, 1):
        plane = torch.full((K, h, w), 9, device=dev, dtype=torch.uint8)            # 9: neither 0, 1 nor 255
        image_bank_update(torch.from_numpy(pred).to(dev), torch.from_numpy(written).to(dev), scale, plane)
        want = np.where(written[:, None, None] != 0, pred * np.uint8(scale), np.uint8(9))
        got = plane.cpu().numpy()
        assert np.array_equal(got, want) and (got[written != 0] != 9).all() and (got[written == 0] == 9).all()


def test_two_refreshes_on_one_stream_give_identical_bytes(dev):
    from aide_amd.labelbank import ImageLabelBank
    rng = np.random.RandomState(8)
    orig, labs = _random_case(rng, 300, 16, 16)
    l1, l2 = (torch.from_numpy(a).to(dev) for a in labs[:2])
    banks = [ImageLabelBank(torch.from_numpy(orig).to(dev), form='kidney', update_percent=0.3) for _ in range(2)]
    for b in banks:
        b.refresh_from_labels(l1, l2, 0, 5, batch_size=64)
    a, b = banks
    for name in ('bank', '_sums', '_dice', 'rank', 'written', '_pred'):
        assert torch.equal(getattr(a, name), getattr(b, name)), name
    # the same bank again, gate closed: the same scores from the same (rewritten) planes twice
    a.refresh_from_labels(l1, l2, 10, 5)
    first = [getattr(a, n).clone() for n in ('_sums', '_dice', 'rank', 'written', 'bank')]
    a.refresh_from_labels(l1, l2, 10, 5)
    assert all(torch.equal(x, getattr(a, n)) for x, n in zip(first, ('_sums', '_dice', 'rank', 'written', 'bank')))


def test_no_host_synchronisation(dev):
    """evaluation, ranking, update and the next targets complete with synchronising calls forbidden; image_dice() is the
    one copy"""
    from aide_amd.labelbank import ImageLabelBank
    rng = np.random.RandomState(4)
    orig, labs = _random_case(rng, 40, 32, 32)
    l1, l2 = (torch.from_numpy(a).to(dev) for a in labs[:2])
    bank = ImageLabelBank(torch.from_numpy(orig).to(dev), labelled=[2], form='breast')
    idx = torch.arange(4, device=dev)
    before = bank.bank.clone()
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode('error')
    try:
        bank.refresh_from_labels(l1, l2, 0, 5)
        t = bank.targets(idx, 1)
        with pytest.raises(RuntimeError):
            bank.image_dice()
    finally:
        torch.cuda.set_sync_debug_mode('default')
    assert tuple(t.shape) == (4, 32, 32) and not torch.equal(bank.bank, before)
    assert tuple(bank.image_dice().shape) == (2, 40)


@pytest.mark.parametrize('form', ['breast', 'kidney'])
def test_refresh_equals_per_image_prediction_and_the_host_rule(dev, form):
    from aide_amd.inference import predict_labels
    from aide_amd.labelbank import ImageLabelBank
    from aide_amd.models_singlemodalinput import UNet
    from aide_amd.synthetic import chaos_cases
    torch.manual_seed(5)
    nets = [UNet(2).to(dev) for _ in range(2)]
    for net in nets:
        net.eval()
    K = 10
    cs = chaos_cases(K, 32, seed=3, slices=(1, 1), labelled=(0, 5), single_modal=True)
    x = cs['inphase'].to(dev)
    bank = ImageLabelBank(cs['initial'].to(dev), labelled=cs['labelled'], form=form, update_percent=0.4)
    host = ImageLabelBank(cs['initial'].numpy(), labelled=cs['labelled'], form=form, update_percent=0.4)
    assert bank.refresh(nets[0], nets[1], x, 0, 1, batch_size=4)
    # per image, batch size 1, as the reference's loop predicts
    labs = [torch.cat([predict_labels(net, x[k:k + 1], batch_size=1) for k in range(K)]).cpu().numpy() for net in nets]
    host.refresh_from_labels(labs[0], labs[1], 0, 1)
    assert np.array_equal(bank._pred.cpu().numpy(), np.stack(labs).astype(np.uint8))
    assert np.array_equal(bank.image_dice().numpy().view(np.uint32), host.image_dice().numpy().view(np.uint32))
    assert np.array_equal(bank.rank.cpu().numpy(), host.rank) and np.array_equal(bank.written.cpu().numpy(), host.written)
    assert np.array_equal(bank.bank.cpu().numpy(), host.bank)


def _mirror(form):
    import importlib
    return importlib.import_module('aide_amd.train_files.' + ('trainkidney_proposed_mask1' if form == 'kidney' else
                                                              'trainbreast_dataset3_proposed_272cases25labeled'))


@pytest.mark.parametrize('form', ['kidney', 'breast'])
def test_train_with_refresh(dev, monkeypatch, caplog, form):
    import logging
    from aide_amd.synthetic import chaos_cases
    mod = _mirror(form)
    monkeypatch.setattr(mod, 'REFRESH_LABELS', [True])
    monkeypatch.setattr(mod, 'REFRESH_IMAGES', [12])
    args = mod.parse_args(['--batch_size', '4', '--img_size', '32', '--num_epoch', '3', '--steps_per_epoch', '2',
                           '--warmup_epoch', '2', '--checkpoint', '', '--update_percent', '0.5']
                          + (['--resumefile', ''] if form == 'kidney' else []))
    with caplog.at_level(logging.INFO):
        n1, n2 = mod.Train(args)
    assert all(torch.isfinite(p).all() for p in list(n1.parameters()) + list(n2.parameters()))
    assert sum('6 masks modified for net1' in r.getMessage() for r in caplog.records) == 2       # epochs 1, 2: gate open; 3: closed
    assert sum('6 masks modify for net2' in r.getMessage() for r in caplog.records) == 2
    bank = mod.LAST_BANK[0]
    assert bank.form == form and bank.K == 12 and bank.n_select == 6
    cs = chaos_cases(12, 32, seed=args.torch_seed * 7919 + 31, slices=(1, 1), labelled=(0, 5), single_modal=True)
    init = cs['initial'].to(dev)
    flags = bank.modified.cpu().numpy()
    assert flags.sum() >= 1
    for n in (0, 1):
        for k in range(12):
            same = torch.equal(bank.bank[n, k], init[k])
            if form == 'breast' and k in cs['labelled']:
                assert same and not flags[n, k]
            elif not same:
                assert flags[n, k]
            if flags[n, k]:
                assert set(torch.unique(bank.bank[n, k]).tolist()) <= ({0, 255} if form == 'breast' else {0, 1})
    assert torch.equal(bank.original, init)


_OFF_SCRIPT = r'''
import sys
sys.path.insert(0, %r)
import importlib
import torch
if %d:
    import aide_amd.labelbank  # noqa: F401
mod = importlib.import_module('aide_amd.train_files.%s')
core = importlib.import_module('aide_amd.train_files.trainchaos_proposed_30cases1labeled')
losses = []
step = core.coteach_step
def rec(*a, **k):
    r = step(*a, **k)
    losses.append((r['loss1'], r['loss2']))
    return r
core.coteach_step = rec
assert mod.REFRESH_LABELS == [False]
args = mod.parse_args(['--batch_size', '4', '--img_size', '64', '--num_epoch', '1', '--steps_per_epoch', '2', '--warmup_epoch', '2',
                       '--checkpoint', ''] + %r)
mod.Train(args)
print('LOSSES', ' '.join('%%08x' %% (l.detach().cpu().view(torch.int32).item() & 0xffffffff) for pair in losses for l in pair))
'''

_MIRRORS = ['trainbreast_dataset3_proposed_272cases25labeled', 'trainkidney_proposed_mask1']


@pytest.mark.parametrize('name', _MIRRORS)
def test_switch_off_is_unchanged(dev, name):
    """switch off, a 1-epoch, 2-step Train in fresh processes: the mirror with and without aide_amd.labelbank imported, and
    the shared loop called the way the mirrors called it before this feature (`Train(args, variant=...)`, no image_refresh
    argument), give the same losses bit for bit: nothing of the per-image bank is reached"""
    extra = ['--resumefile', ''] if 'kidney' in name else []
    outs = []
    for with_bank in (0, 1, 2):
        script = _OFF_SCRIPT % (ROOT, with_bank, name, extra)
        if with_bank == 2:
            script = script.replace('mod.Train(args)', "core.Train(args, variant=%r)" % ('kidney' if 'kidney' in name else 'breast'))
        r = subprocess.run([sys.executable, '-c', script], capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stderr[-2000:]
        line = [ln for ln in r.stdout.splitlines() if ln.startswith('LOSSES')]
        assert len(line) == 1 and len(line[0].split()) == 5, r.stdout[-500:]
        outs.append(line[0])
    assert outs[0] == outs[1] == outs[2], outs
