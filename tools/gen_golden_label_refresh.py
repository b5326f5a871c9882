"""Writes tests/golden/g23_label_refresh.npz: the pseudo-label rewrite as the reference runs it.

    python tools/gen_golden_label_refresh.py

The `if (epoch + 1) <= args.warmup_epoch or (epoch + 1) % 10 == 0:` statement of the epoch loop of the reference's
train_files/trainchaos_proposed_30cases1labeled.py (:528-575) is taken out of the script's syntax tree and executed, with its
own `makefolder`, in a namespace that holds a temporary directory, a stand-in `train_dataset` with the three file lists,
`train_cases`, `label_cases`, `generatedmask1/2`, `traincasedices1/2`, `args.warmup_epoch` and `epoch`.  The case Dice
values are the script's own `Dice3d_fn` of the generated mask against plane 1 of the one-hot of the case's CURRENT mask
files, stored into a `torch.zeros(K)` tensor as :488 does; the mask files are read back with PIL + `one_hot_mask` the way
datasetchaos_proposed/dataset.py:37-105 reads them (`_net1.png` / `_net2.png` when present, the original mask otherwise).
The generated masks are single blobs, i.e. already filtered: skimage is not needed.

Scenarios: K = 9 cases over the epochs 3, 25, 30 (1-based) with warm-up 20 in ONE directory (open, closed, open gate;
the targets of a later epoch are the files an earlier one wrote), and K = 3 (int(0.75) = 0: nothing is selected).
Case 0 is labelled and made network 1's worst case in the first epoch; case 8 has an empty label and empty predictions
(Dice 0 / 0 = NaN); cases 5 and 6 are copies of each other (equal Dice).  `Tensor.sort()` is not stable, so only the
selected SET is recorded as a fact, and the generator asserts that the Dice values on both sides of the selection boundary
differ in every recorded epoch."""
import ast
import os
import sys
import tempfile
import types
import warnings

sys.dont_write_bytecode = True
import numpy as np
import torch
from PIL import Image

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from oracle.gen_golden import REF, _ref_functions  # noqa: E402

OUT = os.path.join(ROOT, 'tests', 'golden', 'g23_label_refresh.npz')
SCRIPT = os.path.join(REF, 'train_files', 'trainchaos_proposed_30cases1labeled.py')
PALETTE = [[0], [63], [126], [189], [252]]
H = W = 32


def _refresh_statement():
    """the `if` of :528 -- the one statement of the epoch loop whose test mentions warmup_epoch and whose body saves PNGs"""
    tree = ast.parse(open(SCRIPT).read(), filename=SCRIPT)
    hits = [n for n in ast.walk(tree) if isinstance(n, ast.If) and 'warmup_epoch' in ast.dump(n.test)
            and 'output_pil' in ast.dump(n)]
    assert len(hits) == 1, len(hits)
    return compile(ast.Module(body=[hits[0]], type_ignores=[]), SCRIPT, 'exec'), (hits[0].lineno, hits[0].end_lineno)


class _Log(object):
    def __init__(self):
        self.lines = []

    def info(self, msg, *a):
        self.lines.append(msg % a if a else msg)


def rect(h0, h1, w0, w1, value=1):
    m = np.zeros((H, W), np.uint8)
    m[max(h0, 0):max(h1, 0), max(w0, 0):max(w1, 0)] = value
    return m


def scenario(out, key, case_ids, n_slices, labelled, epochs, warmup, seed):
    one_hot_mask, makefolder, dice3d = _ref_functions(SCRIPT, ['one_hot_mask', 'makefolder', 'Dice3d_fn'], dict(np=np, os=os))
    loader_one_hot, = _ref_functions(os.path.join(REF, 'datasetchaos_proposed', 'dataset.py'), ['one_hot_mask'], dict(np=np))
    code, lines = _refresh_statement()
    rng = np.random.RandomState(seed)
    K = len(case_ids)
    start = np.concatenate([[0], np.cumsum(n_slices)]).astype(np.int64)
    label_cases = [case_ids[k] for k in labelled]
    # the file lists of the csv (datasetchaos_proposed/dataset.py:15-18): labelled cases keep their ground truth under
    # '<case>/T1DUAL/Ground/', the others have a pseudo-label under '<folder>/<case>/'
    inphase, outphase, masks, stems, init = [], [], [], [], []
    for k, cid in enumerate(case_ids):
        for s in range(n_slices[k]):
            stem = 'IMG-0004-%05d' % (2 * s + 2)
            inphase.append('%d/T1DUAL/DICOM_anon/InPhase/%s.dcm' % (cid, stem))
            outphase.append('%d/T1DUAL/DICOM_anon/OutPhase/IMG-0004-%05d.dcm' % (cid, 2 * s + 1))
            masks.append(('%d/T1DUAL/Ground/%s.png' if k in labelled else 'initial_masks/%d/%s.png') % (cid, stem))
            stems.append(stem)
            m = rect(8, 18 + k, 6 + k, 20 + k, 63)                   # liver (a size of its own per case)
            m[2:6, 2:8] = 126                                        # another organ of the palette
            if k in (5, 6):
                m = rect(8, 24, 10, 24, 63)
            if k == 8:
                m = rect(2, 6, 2, 8, 189)                            # no liver at all
            init.append(m)
    init = np.stack(init)
    with tempfile.TemporaryDirectory() as train_root:
        for path, m in zip(masks, init):
            os.makedirs(os.path.dirname(os.path.join(train_root, path)), exist_ok=True)
            Image.fromarray(m, 'L').save(os.path.join(train_root, path))
        folder = 'generated_masks'
        os.makedirs(os.path.join(train_root, folder))          # (the script creates it before its loop)
        ds = types.SimpleNamespace(t1inphase=inphase, t1outphase=outphase, masks=masks)

        def load(n):
            """mask1 / mask2 of every slice as the loader decodes them -> (bytes [S,H,W], one-hot [S,5,H,W])"""
            raw, oh = [], []
            for i, path in enumerate(masks):
                cid = inphase[i].split('/')[2]
                if not cid.isdigit():
                    cid = inphase[i].split('/')[0]
                p1 = os.path.join(train_root, folder, str(cid), path.split('/')[-1].split('.')[0] + '_net%d.png' % n)
                img = Image.open(p1 if os.path.exists(p1) else os.path.join(train_root, path))
                if img.mode != 'L':
                    img = img.convert('L')
                a = np.array(img)
                raw.append(a)
                oh.append(loader_one_hot(np.expand_dims(a, axis=2), PALETTE).transpose([2, 0, 1]))
            return np.stack(raw), np.stack(oh).astype(np.uint8)

        for j, epoch in enumerate(epochs):
            gens, dices = [], []
            for n in (1, 2):
                raw, oh = load(n)
                gen, dice = [], torch.zeros(K)
                for k in range(K):
                    dh, dw, eh, ew = (int(v) for v in rng.randint(-5, 6, 4))
                    if k == 0 and j == 0 and n == 1:
                        dh, dw, eh, ew = 14, 13, 0, 0                 # the labelled case: network 1's worst
                    if k == 6:
                        g = gen[5].copy()[:, :, :n_slices[6]] if n_slices[6] <= n_slices[5] else None
                        assert g is not None
                    elif k == 8:
                        g = np.zeros((H, W, n_slices[k]), np.uint8)
                    else:
                        g = np.stack([rect(8 + dh, 18 + k + dh + eh, 6 + k + dw, 20 + k + dw + ew) for _ in range(n_slices[k])], axis=-1)
                    target = np.stack([oh[s][1] for s in range(start[k], start[k + 1])], axis=-1)
                    with warnings.catch_warnings():
                        warnings.simplefilter('ignore')
                        dice[k] = dice3d(g, target)                  # :488
                    gen.append(g)
                gens.append(gen)
                dices.append(dice)
            log = _Log()
            ns = dict(epoch=epoch, args=types.SimpleNamespace(warmup_epoch=warmup), train_cases=list(case_ids),
                      label_cases=label_cases, train_dataset=ds, train_root=train_root, tempmaskfolder=folder,
                      traincasedices1=dices[0], traincasedices2=dices[1], generatedmask1=gens[0], generatedmask2=gens[1],
                      os=os, np=np, Image=Image, torch=torch, makefolder=makefolder, logging=log)
            exec(code, ns)
            n_select = int(0.25 * K)
            for n in (0, 1):
                d = dices[n].numpy()
                srt = np.sort(np.where(np.isnan(d), np.inf, d))
                if 0 < n_select < K:                                 # the condition: the selected SET does not hang on a tie
                    assert srt[n_select - 1] != srt[n_select], (key, epoch, n, srt)
            files = []
            for dp, _, fs in os.walk(os.path.join(train_root, folder)):
                files += [os.path.relpath(os.path.join(dp, f), os.path.join(train_root, folder)) for f in fs]
            pre = '%s/e%d' % (key, j)
            out[pre + '/epoch'] = np.asarray(epoch, np.int64)
            for n in (0, 1):
                out['%s/gen%d' % (pre, n + 1)] = np.concatenate([g.transpose(2, 0, 1) for g in gens[n]]).astype(np.uint8)
                out['%s/dice%d' % (pre, n + 1)] = dices[n].numpy()
                raw, oh = load(n + 1)
                out['%s/plane%d' % (pre, n + 1)] = raw
                out['%s/onehot%d' % (pre, n + 1)] = oh
                line = [ln for ln in log.lines if ln.endswith('modify for net%d' % (n + 1))]
                mod = eval(line[0][len('Mask '):line[0].index(']') + 1]) if line else []
                out['%s/modify%d' % (pre, n + 1)] = np.asarray(mod, np.int64)
                out['%s/logged%d' % (pre, n + 1)] = np.asarray(len(line), np.int64)
            out[pre + '/files'] = np.asarray(sorted(files) if files else [], dtype='U64')
    out[key + '/init'] = init
    out[key + '/slice_start'] = start
    out[key + '/case_ids'] = np.asarray(case_ids, np.int64)
    out[key + '/labelled'] = np.asarray(labelled, np.int64)
    out[key + '/stems'] = np.asarray(stems, dtype='U32')
    out[key + '/warmup'] = np.asarray(warmup, np.int64)
    out[key + '/n_epochs'] = np.asarray(len(epochs), np.int64)
    out[key + '/ref_lines'] = np.asarray(lines, np.int64)


def main():
    out = {}
    # 0-based epochs 2, 24, 29: (epoch + 1) = 3 (warm-up: open), 25 (closed), 30 (every tenth: open)
    # (the shifts of the predicted rectangles are drawn; the first seed whose epochs all meet the boundary condition is taken)
    for seed in range(23, 123):
        try:
            tmp = {}
            scenario(tmp, 'k9', [1, 2, 3, 5, 8, 10, 13, 19, 21], [3, 5, 1, 4, 2, 4, 4, 6, 3], [0, 4], [2, 24, 29], 20, seed=seed)
        except AssertionError:
            continue
        out.update(tmp)
        out['k9/seed'] = np.asarray(seed, np.int64)
        break
    scenario(out, 'k3', [4, 7, 9], [2, 3, 1], [1], [2], 20, seed=5)
    out['scenarios'] = np.asarray(['k9', 'k3'])
    # what the fixture must show (checked here, on the reference's own output)
    k9 = {k: v for k, v in out.items() if k.startswith('k9/')}
    sel = [[set(k9['k9/e%d/modify%d' % (j, n)].tolist()) for n in (1, 2)] for j in range(3)]
    assert 1 in sel[0][0], 'the labelled case is in network 1\'s worst quarter of the first epoch'
    assert any(a != b for a, b in sel), 'the two networks select different cases somewhere'
    assert all(len(s) == 2 for pair in (sel[0], sel[2]) for s in pair) and k9['k9/e1/logged1'] == 0
    assert np.isnan(k9['k9/e0/dice1'][8]) and k9['k9/e0/dice1'][5] == k9['k9/e0/dice1'][6]
    assert not any(f.startswith('1/') or f.startswith('8/') for f in k9['k9/e2/files'].tolist()), 'labelled cases are never written'
    assert len(out['k3/e0/files']) == 0 and out['k3/e0/logged1'] == 1
    np.savez_compressed(OUT, **out)
    print('wrote %s (%d bytes)' % (OUT, os.path.getsize(OUT)))
    for j in range(3):
        print('k9 epoch', int(k9['k9/e%d/epoch' % j]) + 1, 'modify', sel[j], 'files', len(k9['k9/e%d/files' % j]))


if __name__ == '__main__':
    torch.set_num_threads(1)
    main()
