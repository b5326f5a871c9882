"""-m gpu: the pseudo-label refresh on the device (aide_amd/csrc/eval3d.hip batched entries, aide_amd/csrc/labelbank.hip,
aide_amd/labelbank.py).  The batched filter equals the per-case one and the CPU function byte for byte, the batched sums
equal the per-case sums, the Dice values have the bits of numpy's float64 division rounded to float32, selection / update /
targets reproduce fixture g23 (the reference's own statement, tools/gen_golden_label_refresh.py), `bank.refresh` equals the
per-case chain, and the proposed loop runs with the switch set and is unchanged with it off.  Integer and index results
are exact; nothing here has a floating tolerance."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, 'tests', 'golden', 'g23_label_refresh.npz')


def _starts(ns):
    return np.concatenate([[0], np.cumsum(ns)]).astype(np.int64)


def _check_filter(vols, dev, cpu=True):
    """vols: per case an [S_k,H,W] int64 array (S_k may be 0).  batched == per-case device == CPU, per case, twice"""
    from aide_amd.inference import keep_largest_batched, keep_largest_connected_components
    start = _starts([v.shape[0] for v in vols])
    cat = torch.from_numpy(np.concatenate(vols)).to(dev)
    st = torch.from_numpy(start).to(dev)
    got = keep_largest_batched(cat, st)
    assert got.is_cuda and got.dtype == torch.uint8 and got.shape == cat.shape
    again = keep_largest_batched(cat, st)
    assert torch.equal(got, again)
    got = got.cpu().numpy()
    for k, v in enumerate(vols):
        g = got[start[k]:start[k + 1]].transpose(1, 2, 0)
        if v.shape[0] == 0:
            continue
        one = keep_largest_connected_components(cat[start[k]:start[k + 1]].permute(1, 2, 0)).cpu().numpy()
        assert np.array_equal(g, one), (k, v.shape, int(g.sum()), int(one.sum()))
        if cpu:
            ref = keep_largest_connected_components(v.transpose(1, 2, 0))
            assert np.array_equal(g, ref), (k, v.shape, int(g.sum()), int(ref.sum()))
    return got, start


@pytest.mark.parametrize('density', [0.05, 0.31, 0.7])
def test_batched_filter_random(dev, density):
    rng = np.random.RandomState(int(density * 100) + 1)
    for K, (h, w) in ((1, (13, 7)), (2, (16, 16)), (7, (33, 50)), (40, (24, 40))):
        ns = rng.randint(1, 12, K)
        if K > 2:
            ns[1], ns[K // 2] = 1, 0                        # a one-slice case and an empty one
        _check_filter([(rng.rand(n, h, w) < density).astype(np.int64) for n in ns], dev)


def test_batched_filter_multiclass_and_empty(dev):
    rng = np.random.RandomState(3)
    ns = [5, 1, 9, 17, 4, 6]
    vols = [rng.randint(0, 6, (n, 37, 29)).astype(np.int64) for n in ns]
    vols[2][:] = 0                                          # no positive value: all zeros
    vols[4] = -rng.randint(0, 3, (4, 37, 29)).astype(np.int64)   # negatives only: foreground, but max <= 0
    got, start = _check_filter(vols, dev)
    assert got[start[2]:start[3]].sum() == 0 and got[start[4]:start[5]].sum() == 0
    from aide_amd.inference import keep_largest_batched
    z = torch.zeros(0, 4, 4, dtype=torch.int64, device=dev)
    assert keep_largest_batched(z, torch.zeros(1, dtype=torch.int64, device=dev)).numel() == 0


def test_batched_filter_case_boundary_and_ties(dev):
    # one column through the last slice of case 0 and the first of case 1: 2 + 3 voxels, never 5
    a = np.zeros((3, 20, 20), np.int64)
    b = np.zeros((4, 20, 20), np.int64)
    a[1:, 7, 9] = 1
    b[:3, 7, 9] = 1
    a[0, 2, 2:5] = 1                                        # 3 voxels elsewhere in case 0: the larger blob there
    got, start = _check_filter([a, b], dev)
    assert got[:3].sum() == 3 and got[0, 2, 2:5].all() and got[3:].sum() == 3 and got[3:6, 7, 9].all()
    # equal areas inside a case: the blob whose first voxel comes first in [H,W,S] order, not in [S,H,W] order
    c = np.zeros((5, 20, 20), np.int64)
    c[0, 10, 3:7] = 1                                       # first in [S,H,W] order
    c[4, 2, 3:7] = 1                                        # first in [H,W,S] order (h = 2)
    c[2, 6, 8:12] = 2                                       # another value, same area, between them
    got, _ = _check_filter([b, c, a], dev)
    assert got[4:9].sum() == 4 and got[8, 2, 3:7].all()


def _winding(h, w, cut):
    """A ragged batch of three cases with 9, 13 and 1 slices of h x w (the cases of a batch share the plane).  Case k holds
    one component of value k + 1 that winds through its whole [H,W,S_k] volume (lcc_cases.serpentine in the case's own
    order: rows along s joined along w, planes of h joined at one corner), so it crosses the 16-wide tile borders in h and w
    and the 4-deep chunk borders in s.  cut = 2 or 4: the odd plane near H / cut, which holds nothing but the joint of the
    two halves, is cleared -- in the middle the half that comes first in raster order is the larger one, at a quarter the
    second one is.  -> [(volume [S_k,H,W], voxels of the larger half or of the whole)]"""
    import lcc_cases
    out = []
    for k, s in enumerate((9, 13, 1)):
        v = lcc_cases.serpentine(h, w, s, k + 1)
        keep = int((v != 0).sum())
        if cut:
            at = (h // cut) | 1
            v[at] = 0
            lo, hi = int((v[:at] != 0).sum()), int((v[at:] != 0).sum())
            assert lo > 0 and hi > 0 and (lo > hi) == (cut == 2)
            keep = max(lo, hi)
        out.append((np.ascontiguousarray(v.transpose(2, 0, 1)), keep))
    return out


@pytest.mark.parametrize('cut', [0, 2, 4], ids=['whole', 'middle', 'quarter'])
def test_batched_filter_serpentine(dev, cut):
    """planes of 40 x 70, 33 x 18 and 17 x 31: the binary batched entry against the CPU function (and the per-case device
    call), the per-class batched entry against the flood fill of lcc_cases -- the whole component is kept, and of a cut one
    the larger half"""
    import lcc_cases
    from aide_amd.inference import keep_largest_batched
    for h, w in ((40, 70), (33, 18), (17, 31)):
        vols, keeps = zip(*_winding(h, w, cut))
        got, start = _check_filter(list(vols), dev)
        per_class = keep_largest_batched(torch.from_numpy(np.concatenate(vols)).to(dev), torch.from_numpy(start).to(dev),
                                         num_classes=4).cpu().numpy()
        for k, v in enumerate(vols):
            a, b = start[k], start[k + 1]
            want = lcc_cases.flood_fill(v.transpose(1, 2, 0), 4)[0].transpose(2, 0, 1)
            assert int((want != 0).sum()) == keeps[k]
            assert np.array_equal(per_class[a:b], want), (h, w, k, int((per_class[a:b] != 0).sum()), keeps[k])
            assert np.array_equal(got[a:b], want != 0), (h, w, k, int(got[a:b].sum()), keeps[k])
            if not cut:
                assert np.array_equal(per_class[a:b], v)


def test_batched_filter_partial_slice_table(dev):
    """S_total = 7 with slice_start = [0, 3, 5]: slices 5 and 6 belong to no case, and their workspace words are neither read
    nor written.  The workspace is pre-filled with valid but wrong words, every parent word 0 and every area word 1: an
    uncovered node that the count stage visited would add its area to root 0, the first voxel of case 0.  Case 0 holds two
    blobs, one of them at node 0.  With equal areas the blob at node 0 wins the tie with or without such additions; with the
    blob at node 0 one voxel smaller, a single uncovered node counted into root 0 flips the winner.  Both, for the binary and
    the per-class entry: slices [0, 5) against the CPU functions and the per-case device calls.  Slices 5 and 6 of `out`
    are not read."""
    from aide_amd._lib import lib, check
    from aide_amd.ops import ptr, stream_ptr
    from aide_amd.inference import keep_largest_connected_components, keep_largest_per_class
    S, H, W, K, C = 7, 20, 37, 2, 3
    n, covered = S * H * W, 5 * H * W
    start = [0, 3, 5]
    table = torch.tensor(start, dtype=torch.int64, device=dev)
    rng = np.random.RandomState(21)
    for smaller in (0, 1):
        lab = np.zeros((S, H, W), np.int64)
        lab[0, 0, 0:6 - smaller] = 1                        # case 0, voxels (h, w, s) = (0, 0 .. 5, 0): the blob of node 0
        lab[1:3, 17, 30:33] = 1                             # case 0: 6 voxels across the tile border at w = 32
        lab[3:5] = rng.randint(0, 3, (2, H, W))             # case 1
        lab[5:] = 1                                         # no case
        v = torch.from_numpy(lab).to(dev)
        for classes in (False, True):
            size = lib.aide_lcc3d_classes_batched_ws_bytes(n, K, C) if classes else lib.aide_lcc3d_batched_ws_bytes(n, K)
            ws = torch.zeros(size // 4, device=dev, dtype=torch.int32)
            ws[n:2 * n] = 1
            out = torch.full((S, H, W), 0xEE, device=dev, dtype=torch.uint8)
            if classes:
                check(lib.aide_keep_largest_cc3d_classes_batched(ptr(v), ptr(table), K, S, H, W, C, ptr(out), ptr(None),
                                                                 ptr(ws), stream_ptr()), 'keep_largest_cc3d_classes_batched')
            else:
                check(lib.aide_keep_largest_cc3d_batched(ptr(v), ptr(table), K, S, H, W, ptr(out), ptr(ws), stream_ptr()),
                      'keep_largest_cc3d_batched')
            got = out[:5].cpu().numpy()
            for a, b in zip(start, start[1:]):
                one, one_dev = lab[a:b].transpose(1, 2, 0), v[a:b].permute(1, 2, 0)
                if classes:
                    want, single = keep_largest_per_class(one, C), keep_largest_per_class(one_dev, C)
                else:
                    want, single = keep_largest_connected_components(one), keep_largest_connected_components(one_dev)
                assert np.array_equal(got[a:b].transpose(1, 2, 0), want), (smaller, classes, a, int(got[a:b].sum()))
                assert np.array_equal(single.cpu().numpy(), want), (smaller, classes, a)
            assert int(got[:3].sum()) == 6 and bool(got[0, 0, 0]) == (not smaller)
            words = ws.cpu().numpy()                        # the words of the uncovered nodes are as they were
            assert not words[covered:n].any() and (words[n + covered:2 * n] == 1).all()


def test_batched_filter_full_size(dev):
    rng = np.random.RandomState(9)
    ns = [33, 30, 35, 1, 36, 33]
    _check_filter([(rng.rand(n, 256, 256) < 0.31).astype(np.int64) for n in ns], dev)
    _check_filter([(rng.rand(100, 512, 512) < 0.31).astype(np.int64)], dev)
    # smooth blobs, as a network predicts them
    yy, xx = np.mgrid[0:256, 0:256]
    vols = []
    for n in (33, 29, 36):
        v = np.zeros((n, 256, 256), np.int64)
        for s in range(n):
            r = 40 * np.sin(np.pi * (s + 1) / (n + 1))
            v[s] = ((yy - 120) ** 2 + (xx - 90) ** 2 < r * r) | ((yy - 200) ** 2 + (xx - 200) ** 2 < 64)
        vols.append(v)
    _check_filter(vols, dev)


def test_batched_sums_and_dice_bits(dev):
    from aide_amd.inference import evaluate_label_maps, case_scores
    rng = np.random.RandomState(12)
    for (h, w) in ((32, 32), (13, 7)):                      # 16-byte rows and the byte path
        ns = [4, 1, 0, 7, 3, 2, 5]
        start = _starts(ns)
        lab = (rng.rand(start[-1], h, w) < 0.4).astype(np.int64)
        bank = np.asarray([0, 63, 126, 189, 252], np.uint8)[rng.randint(0, 5, lab.shape)]
        lab[start[4]:start[5]] = 0                          # empty prediction ...
        bank[start[4]:start[5]] = 126                       # ... against an empty label: 0 / 0
        lab[start[5]:start[6]] = 0                          # empty prediction, non-empty label: Dice 0
        r = evaluate_label_maps(torch.from_numpy(lab).to(dev), torch.from_numpy(start).to(dev), torch.from_numpy(bank).to(dev),
                                keep_largest=False)
        sums, dice = r['sums'].cpu().numpy(), r['dice'].cpu().numpy()
        for k in range(len(ns)):
            p, t = lab[start[k]:start[k + 1]], (bank[start[k]:start[k + 1]] == 63).astype(np.int64)
            assert sums[k].tolist() == [p.size, int((p * t).sum()), int(p.sum()), int(t.sum())]
            if p.size:
                s = case_scores(torch.from_numpy(p).to(dev), torch.from_numpy(t).to(dev))       # aide_case_confusion
                assert (s['TP'], s['TP'] + s['FP'], s['TP'] + s['FN']) == tuple(sums[k][1:].tolist())
            with np.errstate(invalid='ignore'):
                want = np.float32(np.float64(2 * sums[k][1]) / np.float64(sums[k][2] + sums[k][3]))
            assert (np.isnan(want) and np.isnan(dice[k])) or want.view(np.uint32) == dice[k:k + 1].view(np.uint32)[0]
        assert np.isnan(dice[[2, 4]]).all() and dice[5] == 0.0
    # values that need the fp64 division: float32 division of the rounded operands would differ
    big = np.zeros((1, 4), np.int64)
    big[0] = [0, 16777217, 16777217, 50331653]
    from aide_amd._lib import lib, check
    from aide_amd.ops import ptr, stream_ptr
    sums = torch.from_numpy(big).to(dev)
    d = torch.empty(1, device=dev)
    rk = torch.empty(1, device=dev, dtype=torch.int32)
    sel = torch.empty(1, device=dev, dtype=torch.uint8)
    check(lib.aide_label_refresh_select(ptr(sums), None, 1, 1, ptr(d), ptr(rk), ptr(sel), stream_ptr()), 'select')
    want = np.float32(np.float64(2 * 16777217) / np.float64(16777217 + 50331653))
    assert d.cpu().numpy().view(np.uint32)[0] == want.view(np.uint32) and rk.item() == 0 and sel.item() == 1


def test_selection_update_targets_against_g23(dev):
    sys.path.insert(0, os.path.join(ROOT, 'tests'))
    from test_label_refresh_host import make_bank
    g = np.load(GOLD)
    for key in ('k9', 'k3'):
        bank = make_bank(g, key, device=dev)
        host = make_bank(g, key)
        S = int(g[key + '/slice_start'][-1])
        warm = int(g[key + '/warmup'])
        for j in range(int(g[key + '/n_epochs'])):
            pre = '%s/e%d' % (key, j)
            epoch = int(g[pre + '/epoch'])
            l1, l2 = (torch.from_numpy(g['%s/gen%d' % (pre, n)]).to(dev) for n in (1, 2))
            wrote = bank.refresh_from_labels(l1, l2, epoch, warm, keep_largest=False)
            host.refresh_from_labels(g[pre + '/gen1'], g[pre + '/gen2'], epoch, warm, keep_largest=False)
            assert wrote == bool(g[pre + '/logged1'])
            dice = bank.case_dice().numpy()
            for n in (1, 2):
                ref = g['%s/dice%d' % (pre, n)]
                assert np.array_equal(np.isnan(dice[n - 1]), np.isnan(ref))
                assert np.array_equal(dice[n - 1][~np.isnan(ref)].view(np.uint32), ref[~np.isnan(ref)].view(np.uint32))
                if wrote:
                    assert sorted(bank.modify_list(n)) == sorted(g['%s/modify%d' % (pre, n)].tolist())
                assert np.array_equal(bank.bank[n - 1].cpu().numpy(), g['%s/plane%d' % (pre, n)])
                t = bank.targets(torch.arange(S, device=dev), n)
                assert t.dtype == torch.int64 and np.array_equal(t.cpu().numpy(), g['%s/onehot%d' % (pre, n)].astype(np.int64))
                idx = [S - 1, 0, 0, S // 2]
                assert torch.equal(bank.targets(idx, n), t[idx])
            # the numpy bank agrees in everything, the order inside the ranking included
            assert np.array_equal(bank.rank.cpu().numpy(), host.rank) and np.array_equal(bank.selected.cpu().numpy(), host.selected)
            assert np.array_equal(bank.modified.cpu().numpy(), host.modified)


def test_boundary_tie_follows_the_documented_rule(dev):
    """equal Dice on both sides of the boundary: the lower case index is selected; NaN ranks last (this project's rule)"""
    from aide_amd.labelbank import PseudoLabelBank
    K, h = 8, 16
    init = np.zeros((K, h, h), np.uint8)
    init[:, 4:12, 4:12] = 63
    init[6] = 0
    lab = np.zeros((K, h, h), np.int64)
    lab[:, 4:12, 4:8] = 1                                   # every case: Dice 2 * 32 / 96
    lab[6] = 0                                              # NaN
    lab[7, 4:12, 4:12] = 1                                  # Dice 1
    bank = PseudoLabelBank(torch.from_numpy(init).to(dev), list(range(K + 1)), [0])
    assert bank.n_select == 2
    bank.refresh_from_labels(torch.from_numpy(lab).to(dev), torch.from_numpy(lab).to(dev), 0, 1)
    assert bank.rank[0].tolist() == [0, 1, 2, 3, 4, 5, 7, 6]
    assert bank.selected[0].tolist() == [0, 1, 0, 0, 0, 0, 0, 0]      # case 0 is labelled: skipped, its slot not handed on
    assert bank.modify_list(1) == [0, 1]
    out = bank.bank.cpu().numpy()
    want = init.copy()
    want[1] = lab[1] * 63
    assert np.array_equal(out[0], want) and np.array_equal(out[1], want)


def _nets(dev, kind):
    from aide_amd.models_singlemodalinput import UNet
    from aide_amd.models_twomodalinputs import fuseunet
    torch.manual_seed(5)
    nets = [(fuseunet(2) if kind == 'fuseunet' else UNet(2)).to(dev) for _ in range(2)]
    for net in nets:
        net.eval()
    return nets


def _host_rule(dices, labelled, n_select):
    d = torch.zeros(len(dices))
    for k, v in enumerate(dices):
        d[k] = v                                            # a numpy float64 into a float32 tensor (:488)
    _, order = d.sort(stable=True)                          # ascending, NaN last, the lower index first among equals
    return d, [int(k) for k in order[:n_select] if int(k) not in labelled]


@pytest.mark.parametrize('kind', ['fuseunet', 'UNet'])
def test_refresh_equals_the_per_case_chain(dev, kind):
    from aide_amd.inference import predict_case, predict_labels, case_scores, keep_largest_connected_components
    from aide_amd.labelbank import PseudoLabelBank
    from aide_amd.synthetic import chaos_cases
    single = kind == 'UNet'
    nets = _nets(dev, kind)
    # (a) every case 4 slices, forward batches of 4: the batched pass and the per-case loop run the same forward batches
    # (b) ragged cases: the forward once, the per-case chain from the label maps onward
    for ragged in (False, True):
        cs = chaos_cases(8, 32, seed=3 + ragged, slices=(1, 6) if ragged else (4, 4), labelled=(0, 5), single_modal=single)
        st = cs['slice_start']
        inputs = tuple(x.to(dev) for x in ((cs['inphase'],) if single else (cs['inphase'], cs['outphase'])))
        bank = PseudoLabelBank(cs['initial'].to(dev), st, cs['labelled'])
        before = bank.bank.clone()
        assert bank.refresh(nets[0], nets[1], inputs, 0, 1, batch_size=4)
        dice = bank.case_dice()
        for n, net in enumerate(nets):
            labels = predict_labels(net, *inputs, batch_size=4)
            ds, preds = [], []
            for k in range(8):
                a, b = st[k], st[k + 1]
                if ragged:
                    pred = keep_largest_connected_components(labels[a:b].permute(1, 2, 0))
                else:
                    pred = predict_case(net, *[x[a:b] for x in inputs], batch_size=4, keep_largest=True, numpy=False)
                tgt = (before[n, a:b] == 63).to(torch.int64).permute(1, 2, 0)
                ds.append(case_scores(pred, tgt)['Dice'])
                preds.append(pred)
            d, chosen = _host_rule(ds, cs['labelled'], 2)
            assert torch.equal(d.view(torch.int32)[~d.isnan()], dice[n].view(torch.int32)[~d.isnan()])
            assert torch.equal(d.isnan(), dice[n].isnan())
            want = before[n].clone()
            for k in chosen:
                want[st[k]:st[k + 1]] = (preds[k] * 63).permute(2, 0, 1)
            assert torch.equal(bank.bank[n], want)
            assert sorted(torch.nonzero(bank.selected[n]).flatten().tolist()) == sorted(chosen)


def test_no_host_synchronisation(dev):
    """evaluation, ranking, update and the next targets complete with synchronising calls forbidden; case_dice() is the
    one copy"""
    from aide_amd.labelbank import PseudoLabelBank
    rng = np.random.RandomState(4)
    ns = [3, 5, 2, 6, 1, 4, 4, 3]
    start = _starts(ns)
    init = torch.from_numpy(np.asarray([0, 63], np.uint8)[rng.randint(0, 2, (start[-1], 32, 32))]).to(dev)
    l1, l2 = (torch.from_numpy((rng.rand(start[-1], 32, 32) < 0.5).astype(np.int64)).to(dev) for _ in range(2))
    bank = PseudoLabelBank(init, start.tolist(), [2])
    idx = torch.arange(4, device=dev)
    before = bank.bank.clone()
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode('error')
    try:
        bank.refresh_from_labels(l1, l2, 0, 5)
        t = bank.targets(idx, 1)
        with pytest.raises(RuntimeError):
            bank.case_dice()
    finally:
        torch.cuda.set_sync_debug_mode('default')
    assert tuple(t.shape) == (4, 5, 32, 32) and not torch.equal(bank.bank, before)
    assert tuple(bank.case_dice().shape) == (2, 8)


def test_train_with_refresh(dev, monkeypatch, caplog):
    import logging
    from aide_amd.synthetic import chaos_cases
    from aide_amd.train_files import trainchaos_proposed_30cases1labeled as mod
    monkeypatch.setattr(mod, 'REFRESH_LABELS', [True])
    monkeypatch.setattr(mod, 'REFRESH_CASES', [8])
    args = mod.parse_args(['--batch_size', '4', '--img_size', '32', '--num_epoch', '2', '--steps_per_epoch', '2',
                           '--warmup_epoch', '2', '--checkpoint', ''])
    with caplog.at_level(logging.INFO):
        n1, n2 = mod.Train(args)
    assert all(torch.isfinite(p).all() for p in list(n1.parameters()) + list(n2.parameters()))
    assert sum('modify for net1' in r.getMessage() for r in caplog.records) == 2
    assert sum('modify for net2' in r.getMessage() for r in caplog.records) == 2
    bank = mod.LAST_BANK[0]
    cs = chaos_cases(8, 32, seed=args.torch_seed * 7919 + 29)
    st, init = cs['slice_start'], cs['initial'].to(dev)
    mod_flags = bank.modified.cpu().numpy()
    assert mod_flags.sum() >= 1
    for n in (0, 1):
        for k in range(8):
            same = torch.equal(bank.bank[n, st[k]:st[k + 1]], init[st[k]:st[k + 1]])
            if k in cs['labelled']:
                assert same and not mod_flags[n, k]
            elif not same:
                assert mod_flags[n, k]
        vals = torch.unique(bank.bank[n]).tolist()
        assert set(vals) <= {0, 63}


_OFF_SCRIPT = r'''
import sys
sys.path.insert(0, %r)
import torch
if %d:
    import aide_amd.labelbank  # noqa: F401
from aide_amd.train_files import trainchaos_proposed_30cases1labeled as mod
losses = []
step = mod.coteach_step
def rec(*a, **k):
    r = step(*a, **k)
    losses.append((r['loss1'], r['loss2']))
    return r
mod.coteach_step = rec
assert mod.REFRESH_LABELS == [False]
args = mod.parse_args(['--batch_size', '4', '--img_size', '64', '--num_epoch', '1', '--steps_per_epoch', '2', '--warmup_epoch', '2',
                       '--checkpoint', ''])
mod.Train(args)
print('LOSSES', ' '.join('%%08x' %% (l.detach().cpu().view(torch.int32).item() & 0xffffffff) for pair in losses for l in pair))
'''


# loss1, loss2 of the two steps of that run on the commit before this feature, recorded on an MI355X (two fresh processes
# gave the same bits there, and so did two of this tree)
_PARENT_LOSSES = 'LOSSES 40531064 404a5939 405a1d35 40561e2c'


def test_switch_off_is_unchanged(dev):
    """switch off, a 1-epoch, 2-step Train: the losses of the loop before this feature, bit for bit, with and without
    aide_amd.labelbank imported (each run in a fresh process)"""
    outs = []
    for with_bank in (0, 1):
        r = subprocess.run([sys.executable, '-c', _OFF_SCRIPT % (ROOT, with_bank)], capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stderr[-2000:]
        line = [ln for ln in r.stdout.splitlines() if ln.startswith('LOSSES')]
        assert len(line) == 1 and len(line[0].split()) == 5, r.stdout[-500:]
        outs.append(line[0])
    assert outs[0] == outs[1], outs
    assert outs[0] == _PARENT_LOSSES, outs
