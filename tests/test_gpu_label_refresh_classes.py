"""-m gpu: the per-class (multi-organ) pseudo-label refresh on the device (the per-class entries of aide_amd/csrc/labelbank.hip,
`evaluate_label_maps(num_classes=C)`, `PseudoLabelBank(num_classes=C)`).  Every device result is compared with the host
definition (`case_class_counts`, `case_dice_rule_classes`, the numpy bank) on the same inputs: integers and bytes are equal,
floats are equal in their bit patterns (NaN included: both sides make it by the same 0 / 0 division).  The shapes are the
smallest that reach each path: the scalar and the 16-byte form, a misaligned view, several workgroups per case, ragged and
empty cases, one case and more cases than one wave."""
import numpy as np
import pytest
import torch

import label_refresh_classes_cases as lc

pytestmark = pytest.mark.gpu


def _dev_counts(pred, bank, st, pal, C):
    from aide_amd._lib import lib, check
    from aide_amd.ops import ptr, stream_ptr
    k = st.numel() - 1
    out = torch.full((k, C, 3), -1, device=pred.device, dtype=torch.int64)
    check(lib.aide_case_class_counts_batched(ptr(pred), ptr(bank), ptr(st), k, *pred.shape, ptr(pal), C, ptr(out), stream_ptr()),
          'case_class_counts_batched')
    return out


def _off_by_one(x, dev):
    """the same bytes at an odd device address"""
    flat = torch.zeros(x.size + 1, dtype=torch.uint8, device=dev)
    flat[1:].copy_(torch.from_numpy(x).reshape(-1))
    v = flat[1:].view(x.shape)
    assert v.data_ptr() % 2 == 1 and v.is_contiguous()
    return v


@pytest.mark.parametrize('C', [2, 3, 5, 8])
def test_counts_kernel(dev, C):
    from aide_amd.inference import case_class_counts
    pal = lc.PALETTES[C]
    pal_d = torch.tensor(pal, dtype=torch.int32, device=dev)
    ragged70 = [(3 * k) % 5 for k in range(70)]
    for ns, (h, w), shifted in ((lc.RAGGED, (5, 7), False), (lc.RAGGED, (16, 16), False), (lc.RAGGED, (16, 16), True),
                                ([9, 2], (64, 64), False), ([3], (16, 16), False), ([2], (5, 7), False),
                                (ragged70, (16, 16), False), (ragged70, (3, 5), False)):
        lab, bank, st = lc.random_maps(C + h, ns, h, w, pal)
        want = case_class_counts(lab, bank, st, pal)
        assert np.array_equal(want, lc.loop_counts(lab, bank, st, pal))
        st_d = torch.from_numpy(st).to(dev)
        bank_d = torch.from_numpy(bank).to(dev)
        lab_d = _off_by_one(lab, dev) if shifted else torch.from_numpy(lab).to(dev)
        got = _dev_counts(lab_d, bank_d, st_d, pal_d, C)
        again = _dev_counts(lab_d, bank_d, st_d, pal_d, C)
        assert torch.equal(got, again)                     # integer atomics: the same bytes from call to call
        assert np.array_equal(got.cpu().numpy(), want), (C, ns, h, w, shifted)
        if shifted:                                        # ... and with the bank at the odd address instead
            lab_d, bank_d = torch.from_numpy(lab).to(dev), _off_by_one(bank, dev)
            got = _dev_counts(lab_d, bank_d, st_d, pal_d, C)
            assert np.array_equal(got.cpu().numpy(), want)


@pytest.mark.parametrize('C', [2, 5, 8])
def test_counts_kernel_long_cases(dev, C):
    """The kernel keeps its counters as packed bytes and empties them every 15 vector loads (240 voxels) or 255 scalar
    loads.  A thread walks its case with a stride of grid.x * 256 loads, grid.x = 4 * ceil(hw / 4096) (vector) or
    4 * ceil(hw / 256) (scalar), so it takes ns / 4 loads at 64x64, ns / 64 at 16x16 and ns * 35 / 1024 at 5x7: these cases
    give 20, 17 and 263 loads per thread, past the first flush, with one class at nearly every voxel so that its byte is
    full when the flush comes.  160 slices at 64x64 (40 vector loads) and 15400 at 5x7 (526 scalar loads) pass the second
    flush as well, which a counter of loads that is not set back after the first would miss."""
    from aide_amd.inference import case_class_counts
    pal = lc.PALETTES[C]
    pal_d = torch.tensor(pal, dtype=torch.int32, device=dev)
    for ns, (h, w) in ((80, (64, 64)), (1088, (16, 16)), (7700, (5, 7)), (160, (64, 64)), (15400, (5, 7))):
        lab, bank, st = lc.long_case_maps(C + ns, ns, h, w, pal)
        want = case_class_counts(lab, bank, st, pal)
        assert want[0, C - 1].min() > 0.9 * lab.size
        got = _dev_counts(torch.from_numpy(lab).to(dev), torch.from_numpy(bank).to(dev), torch.from_numpy(st).to(dev), pal_d, C)
        assert np.array_equal(got.cpu().numpy(), want), (C, ns, h, w)
    # two long cases side by side at an odd address: the scalar form on 16-byte planes, 1100 * 256 / 1024 = 275 loads
    lab, bank, _ = lc.long_case_maps(C, 2200, 16, 16, pal)
    st = lc.starts([1100, 1100])
    want = case_class_counts(lab, bank, st, pal)
    st_d = torch.from_numpy(st).to(dev)
    got = _dev_counts(_off_by_one(lab, dev), torch.from_numpy(bank).to(dev), st_d, pal_d, C)
    assert np.array_equal(got.cpu().numpy(), want)


def test_counts_arguments(dev):
    from aide_amd._lib import lib
    from aide_amd.ops import ptr, stream_ptr
    z = torch.zeros(2, 4, 4, dtype=torch.uint8, device=dev)
    st = torch.tensor([0, 2], dtype=torch.int64, device=dev)
    pal = torch.arange(9, dtype=torch.int32, device=dev)
    out = torch.zeros(1, 9, 3, dtype=torch.int64, device=dev)
    for C in (1, 9):
        assert lib.aide_case_class_counts_batched(ptr(z), ptr(z), ptr(st), 1, 2, 4, 4, ptr(pal), C, ptr(out), stream_ptr()) < 0
    assert lib.aide_case_class_counts_batched(ptr(z), ptr(z), ptr(st), 65536, 2, 4, 4, ptr(pal), 2, ptr(out), stream_ptr()) < 0


def _dev_select(counts, labelled, n_select, dev):
    from aide_amd._lib import lib, check
    from aide_amd.ops import ptr, stream_ptr
    k, c = counts.shape[:2]
    cd = torch.empty(k, c, device=dev, dtype=torch.float32)
    dice = torch.empty(k, device=dev, dtype=torch.float32)
    rank = torch.empty(k, device=dev, dtype=torch.int32)
    sel = torch.empty(k, device=dev, dtype=torch.uint8)
    lab = torch.from_numpy(labelled).to(dev) if labelled is not None else None
    cnt = torch.from_numpy(counts).to(dev)
    check(lib.aide_label_refresh_select_classes(ptr(cnt), ptr(lab), k, c, n_select, ptr(cd), ptr(dice), ptr(rank), ptr(sel),
                                                stream_ptr()), 'label_refresh_select_classes')
    return tuple(x.cpu().numpy() for x in (cd, dice, rank, sel))


@pytest.mark.parametrize('K', [1, 257, 4096])
def test_select_kernel(dev, K):
    from aide_amd.inference import case_dice_rule_classes
    for C in (2, 5, 8):
        counts, labelled = lc.rule_counts(K + C, K, C)
        for n_select, lab in ((max(1, K // 4), labelled), (0, None), (K + 3, labelled)):
            want = case_dice_rule_classes(counts, lab, n_select)
            got = _dev_select(counts, lab, n_select, dev)
            for name, a, b in zip(('class_dice', 'dice', 'rank', 'selected'), got, want):
                assert lc.same_bits(a, b), (K, C, n_select, name)
        if K > 1:
            dice, rank = want[1], want[2]
            order = np.argsort(rank)
            n = K // 4
            assert np.isnan(dice).any() and labelled.any()
            assert dice[order[n - 1]] == dice[order[n]]      # a tie across the selection boundary of the first round


def test_select_kernel_limit(dev):
    counts = np.zeros((4097, 2, 3), np.int64)
    with pytest.raises(RuntimeError):
        _dev_select(counts, None, 1, dev)


def test_update_kernel(dev):
    from aide_amd._lib import lib, check
    from aide_amd.ops import ptr, stream_ptr
    C = 5
    pal = lc.PALETTES[C]
    pal_d = torch.tensor(pal, dtype=torch.int32, device=dev)
    lut = np.full(256, pal[0], np.uint8)
    lut[:C] = pal
    ns = [2, 1, 3, 0, 2, 2]
    for (h, w), shifted in (((16, 16), False), ((5, 7), False), ((16, 16), True)):
        lab, bank, st = lc.random_maps(h, ns, h, w, pal)
        assert (lab >= C).any()
        st_d, lab_d = torch.from_numpy(st).to(dev), torch.from_numpy(lab).to(dev)
        for chosen in ([1, 0, 1, 0, 0, 1], [0, 1, 0, 1, 1, 0], [0] * 6, [1] * 6):
            want = bank.copy()
            for k in np.flatnonzero(chosen):
                want[st[k]:st[k + 1]] = lut[lab[st[k]:st[k + 1]]]
            bank_d = _off_by_one(bank, dev) if shifted else torch.from_numpy(bank).to(dev)
            sel = torch.tensor(chosen, dtype=torch.uint8, device=dev)
            check(lib.aide_label_bank_update_classes(ptr(lab_d), ptr(sel), ptr(st_d), len(ns), *lab.shape, ptr(pal_d), C,
                                                     ptr(bank_d), stream_ptr()), 'label_bank_update_classes')
            # the whole plane: the selected cases rewritten, every byte of their unselected neighbours as it was
            assert np.array_equal(bank_d.cpu().numpy(), want), ((h, w), shifted, chosen)


def test_index_targets(dev):
    from aide_amd.labelbank import PseudoLabelBank
    for C, (h, w) in ((5, (16, 16)), (3, (5, 7)), (8, (33, 9))):
        pal = lc.PALETTES[C]
        _, plane, st = lc.random_maps(C, [3, 2], h, w, pal)
        assert not np.isin(plane, pal).all()
        bank = PseudoLabelBank(torch.from_numpy(plane).to(dev), st.tolist(), [], palette=pal)
        host = PseudoLabelBank(plane, st.tolist(), [], palette=pal)
        idx = [4, -1, 0, 5, 2, 2, 1 << 40]
        for ignore in (255, -100):
            got = bank.targets(idx, 2, index=True, ignore_index=ignore)
            assert got.is_cuda and got.dtype == torch.int64 and tuple(got.shape) == (7, h, w)
            got = got.cpu().numpy()
            assert np.array_equal(got, host.targets(idx, 2, index=True, ignore_index=ignore).numpy())
            assert (got[[1, 3, 6]] == ignore).all()
            ok = [0, 2, 4, 5]
            oh = bank.targets([idx[i] for i in ok], 2).cpu().numpy()
            known = oh.sum(1) == 1
            assert np.array_equal(got[ok][known], oh.argmax(1)[known]) and (got[ok][~known] == ignore).all() and (~known).any()


def _refresh_both(dev_bank, host_bank, maps, epoch, warm, dev):
    wrote = dev_bank.refresh_from_labels(*[torch.from_numpy(m).to(dev) for m in maps], epoch, warm)
    assert wrote == host_bank.refresh_from_labels(*maps, epoch, warm)
    assert np.array_equal(dev_bank.bank.cpu().numpy(), host_bank.bank)
    assert lc.same_bits(dev_bank.case_dice().numpy(), host_bank.case_dice().numpy())
    assert np.array_equal(dev_bank.rank.cpu().numpy(), host_bank.rank)
    assert np.array_equal(dev_bank.selected.cpu().numpy(), host_bank.selected)
    assert np.array_equal(dev_bank.modified.cpu().numpy(), host_bank.modified)
    for n in (1, 2):
        assert dev_bank.modify_list(n) == host_bank.modify_list(n)
    return wrote


def test_whole_bank(dev):
    from aide_amd.labelbank import PseudoLabelBank
    from aide_amd.synthetic import chaos_cases, chaos_cases_multiorgan
    C = 5
    cs = chaos_cases_multiorgan(6, C, 32, seed=7, slices=(2, 5), labelled=(0,))
    st = cs['slice_start']
    banks = (PseudoLabelBank(cs['initial'].to(dev), st, cs['labelled'], num_classes=C),
             PseudoLabelBank(cs['initial'].numpy(), st, cs['labelled'], num_classes=C))
    assert _refresh_both(*banks, lc.class_maps(cs, C, seed=1), 0, 1, dev)
    assert lc.same_bits(banks[0].class_dice().numpy(), banks[1].class_dice().numpy())
    assert not np.array_equal(banks[1].bank[0], cs['initial'].numpy())
    assert not _refresh_both(*banks, lc.class_maps(cs, C, seed=2), 1, 1, dev)
    assert lc.same_bits(banks[0].class_dice().numpy(), banks[1].class_dice().numpy())
    assert tuple(banks[0].class_dice().shape) == (2, 6, C)
    # C = 2 on the device: the binary refresh bit for bit
    cs = chaos_cases(8, 32, seed=11, slices=(1, 5), labelled=(0, 5))
    st = cs['slice_start']
    rng = np.random.RandomState(2)
    truth = (cs['truth'].numpy() == 63).astype(np.int64)
    maps = [torch.from_numpy(np.roll(truth, (1 + n, 2), (1, 2)) | (rng.rand(*truth.shape) < 0.03)).to(dev) for n in range(4)]
    two = [PseudoLabelBank(cs['initial'].to(dev), st, cs['labelled'], palette=(0, 63), **kw) for kw in ({}, {'num_classes': 2})]
    for bank in two:
        assert bank.refresh_from_labels(maps[0], maps[1], 0, 1)
    assert lc.same_bits(two[0].case_dice().numpy(), two[1].case_dice().numpy())
    for bank in two:
        assert not bank.refresh_from_labels(maps[2], maps[3], 1, 1)
    assert torch.equal(two[0].bank, two[1].bank) and not torch.equal(two[0].bank[0], cs['initial'].to(dev))
    assert lc.same_bits(two[0].case_dice().numpy(), two[1].case_dice().numpy())
    assert torch.equal(two[0].rank, two[1].rank) and torch.equal(two[0].selected, two[1].selected)
    assert torch.equal(two[0].modified, two[1].modified)


def test_refresh_through_the_networks(dev):
    from aide_amd.inference import predict_case, case_scores, case_dice_rule_classes
    from aide_amd.labelbank import PseudoLabelBank, CHAOS_PALETTE
    from aide_amd.models_singlemodalinput import UNet2
    from aide_amd.synthetic import chaos_cases_multiorgan
    from aide_amd.utils import CoTeachingProposedLoss, pseudo_label_ensemble
    C, K = 3, 8
    pal = CHAOS_PALETTE[:C]
    torch.manual_seed(5)
    nets = [UNet2(num_classes=C).to(dev).eval() for _ in range(2)]
    cs = chaos_cases_multiorgan(K, C, 32, seed=3, slices=(4, 4), labelled=(0, 5))
    st = cs['slice_start']
    x = cs['inphase'].to(dev)
    bank = PseudoLabelBank(cs['initial'].to(dev), st, cs['labelled'], palette=pal, num_classes=C)
    before = bank.bank.clone()
    assert bank.refresh(nets[0], nets[1], (x,), 0, 1, batch_size=4)
    to_class = torch.full((256,), C, dtype=torch.int64, device=dev)
    to_class[list(pal)] = torch.arange(C, device=dev)
    to_byte = torch.tensor(pal, dtype=torch.uint8, device=dev)
    dice, cdice = bank.case_dice().numpy(), bank.class_dice().numpy()
    for n, net in enumerate(nets):
        counts, preds = np.zeros((K, C, 3), np.int64), []
        for k in range(K):
            a, b = st[k], st[k + 1]
            pred = predict_case(net, x[a:b], batch_size=4, keep_largest='per_class', num_classes=C, numpy=False)
            s = case_scores(pred, to_class[before[n, a:b].long()].permute(1, 2, 0), num_classes=C)
            counts[k] = np.stack([s['TP'], s['TP'] + s['FP'], s['TP'] + s['FN']], axis=1)
            preds.append(pred)
        cd, d, rank, sel = case_dice_rule_classes(counts, bank.labelled_host, bank.n_select)
        assert lc.same_bits(dice[n], d) and lc.same_bits(cdice[n], cd)
        assert np.array_equal(bank.rank[n].cpu().numpy(), rank) and np.array_equal(bank.selected[n].cpu().numpy(), sel)
        want = before[n].clone()
        for k in np.flatnonzero(sel):
            want[st[k]:st[k + 1]] = to_byte[preds[k].long()].permute(2, 0, 1)
        assert torch.equal(bank.bank[n], want)
    # the next step: class-index targets from the bank straight into the fused co-teaching loss
    idx = torch.tensor([1, 6, 13, 30], device=dev)
    t1, t2 = (bank.targets(idx, n, index=True) for n in (1, 2))
    assert t1.dtype == torch.int64 and tuple(t1.shape) == (4, 32, 32) and int(t1.max()) < C
    for net in nets:
        net.train()
    o1, o2 = nets[0](x[idx]), nets[1](x[idx])
    pseudo, wmap = pseudo_label_ensemble([o1.detach(), o2.detach()], temperature=1.0)
    l1, l2, _, _ = CoTeachingProposedLoss(keep=2)(o1, o2, t1, t2, pseudo, wmap, pseudo, wmap, 0.25)
    (l1 + l2).backward()
    grads = [p.grad for net in nets for p in net.parameters()]
    assert all(g is not None and torch.isfinite(g).all() for g in grads) and any(float(g.abs().max()) > 0 for g in grads)


def test_no_host_synchronisation(dev):
    """evaluation, ranking, update and the next index targets of a C-class bank complete with synchronising calls forbidden;
    case_dice() / class_dice() are the copies"""
    from aide_amd.labelbank import PseudoLabelBank, CHAOS_PALETTE
    rng = np.random.RandomState(4)
    ns = [3, 5, 2, 6, 1, 4, 4, 3]
    st = lc.starts(ns)
    init = torch.from_numpy(np.asarray(CHAOS_PALETTE, np.uint8)[rng.randint(0, 5, (st[-1], 32, 32))]).to(dev)
    l1, l2 = (torch.from_numpy(rng.randint(0, 5, (st[-1], 32, 32)).astype(np.int64)).to(dev) for _ in range(2))
    bank = PseudoLabelBank(init, st.tolist(), [2], num_classes=5)
    idx = torch.arange(4, device=dev)
    before = bank.bank.clone()
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode('error')
    try:
        bank.refresh_from_labels(l1, l2, 0, 5)
        t = bank.targets(idx, 1, index=True)
        with pytest.raises(RuntimeError):
            bank.class_dice()
    finally:
        torch.cuda.set_sync_debug_mode('default')
    assert tuple(t.shape) == (4, 32, 32) and not torch.equal(bank.bank, before)
    assert tuple(bank.class_dice().shape) == (2, 8, 5) and tuple(bank.case_dice().shape) == (2, 8)
