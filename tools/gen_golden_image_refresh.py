"""Writes tests/golden/g24_image_refresh.npz: the per-image pseudo-label rewrite as the reference runs it.

    python tools/gen_golden_image_refresh.py

The `if (epoch + 1) <= args.warmup_epoch or (epoch + 1) % 10 == 0:` statement of the epoch loops of the reference's
train_files/trainbreast_dataset3_proposed_272cases25labeled.py (:401-438) and train_files/trainkidney_proposed_mask1.py (:404-434)
is taken out of each script's syntax tree and executed, with the script's own `makefolder`, in a namespace that holds a
temporary directory and stand-ins for `train_dataset`, `labeled_cases` / `maskannotations`, `args`, `logging`,
`generatedmask1/2` and `traindices1/2`.  The Dice values are the scripts' own `Dice2d` of the generated mask against the
target the loader would hand out, stored into a `torch.zeros(K)` tensor as :392-393 do.  Breast: the files go through real PIL
(the stand-in `Image` only notes the paths that are saved) and are read back the way datasetbreast_proposed/dataset.py:58-70
reads them (`> 0 -> 1`).  Kidney: a stand-in `sitk` with just GetImageFromArray / WriteImage records the arrays; they are read
back as datasetkidney_proposed/dataset.py:53-61 does (`> 0.5 -> 255`) and go through the reference's own `ToTensor`
(datasetkidney_proposed/transform.py:87-111, executed from its syntax tree), which multiplies every mask by
len(np.unique(original mask)) - 1.  Nothing of the reference's text is written anywhere.

Which target a network is scored against is the scripts' (:380-381): breast network 1 sample[2] (the original mask), network 2
sample[3] (network 1's pseudo-label); kidney network 1 sample[4] (network 2's), network 2 sample[3] (network 1's).

Scenarios at H = W = 32, K = 12 over the epochs 3, 25, 30 (1-based) with warm-up 20 in ONE directory (open, closed, open gate;
later targets are what earlier epochs wrote), breast with update_percent 0.25 and kidney with 0.4, and K = 3 (int(0.75) = 0).
  image 0   breast: labelled, and network 1's prediction misses its target: Dice 0.0, inside the worst quarter, not written
  image 1   empty target and empty predictions: Dice 0.0 (never NaN), ranked worst, NOT written
  image 2   non-empty target, network 2's prediction empty: selected, not written
  image 3   empty original mask, non-empty predictions: Dice 0.0, written
  images 4, 5  copies of each other (equal Dice)
  image 6   original mask constant 255 (kidney: every target of it is zero, whatever its planes hold after the first rewrite)
`Tensor.sort()` is not stable, so only the SET of images written is recorded as a fact, and the generator asserts that the
Dice values on both sides of the selection boundary differ in every recorded epoch."""
import ast
import os
import sys
import tempfile
import types

sys.dont_write_bytecode = True
import numpy as np
import torch
from PIL import Image

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from oracle.gen_golden import REF, _ref_functions  # noqa: E402

OUT = os.path.join(ROOT, 'tests', 'golden', 'g24_image_refresh.npz')
SCRIPTS = {'breast': os.path.join(REF, 'train_files', 'trainbreast_dataset3_proposed_272cases25labeled.py'),
           'kidney': os.path.join(REF, 'train_files', 'trainkidney_proposed_mask1.py')}
KIDNEY_TRANSFORM = os.path.join(REF, 'datasetkidney_proposed', 'transform.py')
H = W = 32


def _refresh_statement(script):
    """the one `if` of the epoch loop whose test mentions warmup_epoch and whose body selects `selected_samples` images"""
    tree = ast.parse(open(script).read(), filename=script)
    hits = [n for n in ast.walk(tree) if isinstance(n, ast.If) and 'warmup_epoch' in ast.dump(n.test)
            and 'selected_samples' in ast.dump(n)]
    assert len(hits) == 1, len(hits)
    return compile(ast.Module(body=[hits[0]], type_ignores=[]), script, 'exec'), (hits[0].lineno, hits[0].end_lineno)


def _ref_class(path, name, glb):
    tree = ast.parse(open(path).read(), filename=path)
    body = [n for n in tree.body if isinstance(n, ast.ClassDef) and n.name == name]
    assert len(body) == 1
    ns = dict(glb)
    exec(compile(ast.Module(body=body, type_ignores=[]), path, 'exec'), ns)
    return ns[name]


class _Log(object):
    def __init__(self):
        self.lines = []

    def info(self, msg, *a):
        self.lines.append(msg % a if a else msg)


class _Dataset(object):
    """what the statement reads of `train_dataset`: its length and the csv columns"""
    def __init__(self, masks, depths):
        self.masks, self.depths = masks, depths

    def __len__(self):
        return len(self.masks)


class _NotingImage(object):
    """PIL's Image for the statement: fromarray / save are PIL's, the saved paths are noted"""
    def __init__(self):
        self.saved = []

    def fromarray(self, a, *args, **kw):
        img, noted = Image.fromarray(a, *args, **kw), self.saved
        save = img.save

        def noting_save(path, *sa, **skw):
            noted.append(path)
            return save(path, *sa, **skw)
        img.save = noting_save
        return img


class _Sitk(object):
    """GetImageFromArray / WriteImage only: the arrays are kept per path"""
    def __init__(self):
        self.volumes, self.saved = {}, []

    def GetImageFromArray(self, a):
        return np.array(a, copy=True)

    def WriteImage(self, img, path):
        self.volumes[path] = img
        self.saved.append(path)


def rect(h0, h1, w0, w1, value=1):
    m = np.zeros((H, W), np.uint8)
    m[max(h0, 0):max(h1, 0), max(w0, 0):max(w1, 0)] = value
    return m


def scenario(out, key, form, K, update_percent, epochs, warmup, seed):
    script = SCRIPTS[form]
    makefolder, dice2d = _ref_functions(script, ['makefolder', 'Dice2d'], dict(np=np, os=os))
    code, lines = _refresh_statement(script)
    to_tensor = _ref_class(KIDNEY_TRANSFORM, 'ToTensor', dict(np=np, torch=torch))() if form == 'kidney' else None
    rng = np.random.RandomState(seed)
    orig = np.stack([rect(8, 18 + k, 6 + k, 20 + k, 255) for k in range(K)])
    if K > 6:
        orig[1] = 0
        orig[3] = 0
        orig[5] = orig[4]
        orig[6] = 255
    labelled = [0]
    if form == 'breast':
        names = ['gt/case00_segmentation.nii.gz'] + ['pseudo/case%02d' % (1 + (k - 1) // 3) for k in range(1, K)]
        depths = [7] + [(k - 1) % 3 + 4 for k in range(1, K)]
        ids_a = [nm.split('/')[-1] for nm in names]
        ids_b = [str(d) for d in depths]
    else:
        names = ['annotator1/vol%02d/slice%03d.nii.gz' % (k // 4, k) for k in range(K)]
        ids_a = [nm.split('/')[-2] for nm in names]
        ids_b = [nm.split('/')[-1].split('.')[0] for nm in names]
    folder = 'generated_masks'
    sitk = _Sitk()
    with tempfile.TemporaryDirectory() as train_root:
        os.makedirs(os.path.join(train_root, folder))             # (the scripts create it before their loops)

        def path_of(k, n):
            if form == 'breast':
                return os.path.join(train_root, folder, ids_a[k], '%s_depth%s_net%d.png' % (ids_a[k], ids_b[k], n))
            return os.path.join(train_root, folder, ids_a[k], '%s_net%d.nii.gz' % (ids_b[k], n))

        def plane(k, n):
            """the bytes behind mask1 / mask2 of image k: the written file, the original mask while there is none"""
            p = path_of(k, n)
            if form == 'breast':
                return np.array(Image.open(p)) if os.path.exists(p) else orig[k]
            return sitk.volumes[p][0].astype(np.uint8) if p in sitk.volumes else orig[k]

        def sample(k):
            """(mask, mask1, mask2) of `train_dataset.__getitem__(k)` without the random transform, as int64 arrays"""
            if form == 'breast':                                   # dataset.py:55-70, transform.py:99-104
                return tuple((a > 0).astype(np.int64) for a in (orig[k], plane(k, 1), plane(k, 2)))
            pil = [Image.fromarray(np.where(a > 0.5, 255, 0).astype(np.uint8)) for a in (orig[k], plane(k, 1), plane(k, 2))]
            img = Image.fromarray(np.zeros((H, W, 3), np.uint8))
            augset = dict(('img%d' % i, img) for i in range(1, 5))
            _, _, m, m1, m2 = to_tensor(img, augset, *pil)
            return m.numpy(), m1.numpy(), m2.numpy()

        for j, epoch in enumerate(epochs):
            samples = [sample(k) for k in range(K)]
            gens, dices = [], []
            for n in (1, 2):
                gen, dice = [], torch.zeros(K)
                for k in range(K):
                    dh, dw, eh, ew = (int(v) for v in rng.randint(-5, 6, 4))
                    g = rect(8 + dh, 18 + k + dh + eh, 6 + k + dw, 20 + k + dw + ew).astype(np.int64)
                    if K > 6:
                        if k == 0 and n == 1 and form == 'breast':
                            g = rect(0, 4, 26, 32).astype(np.int64)          # misses its target
                        if k == 1 or (k == 2 and n == 2):
                            g[:] = 0
                        if k == 5:
                            g = gen[4].reshape(H, W).copy()
                    if form == 'kidney':
                        g = g[None]                                          # :391 `output1.unsqueeze(dim=0).numpy()`
                    s = samples[k]
                    target = (s[0] if n == 1 else s[1]) if form == 'breast' else (s[2] if n == 1 else s[1])    # :380-381
                    dice[k] = dice2d(g, target)                              # :392-395
                    gen.append(g)
                gens.append(gen)
                dices.append(dice)
            log, noting = _Log(), _NotingImage()
            sitk.saved = []
            ns = dict(epoch=epoch, args=types.SimpleNamespace(warmup_epoch=warmup, update_percent=update_percent, maskidentity=1),
                      train_dataset=_Dataset(names, depths if form == 'breast' else None),
                      labeled_cases=[names[k] for k in labelled], maskannotations={'1': names}, train_root=train_root,
                      tempmaskfolder=folder, traindices1=dices[0], traindices2=dices[1], generatedmask1=gens[0],
                      generatedmask2=gens[1], evaltrainavgdicetemp=0.0, os=os, np=np, Image=noting, torch=torch, sitk=sitk,
                      makefolder=makefolder, logging=log)
            exec(code, ns)
            n_select = int(update_percent * K)
            for n in (0, 1):
                srt = np.sort(dices[n].numpy())
                if 0 < n_select < K:                                 # the condition: the written SET does not hang on a tie
                    assert srt[n_select - 1] != srt[n_select], (key, epoch, n, srt)
            saved = noting.saved if form == 'breast' else sitk.saved
            pre = '%s/e%d' % (key, j)
            out[pre + '/epoch'] = np.asarray(epoch, np.int64)
            out[pre + '/logged'] = np.asarray(len(log.lines), np.int64)
            after = [sample(k) for k in range(K)]
            for n in (1, 2):
                out['%s/gen%d' % (pre, n)] = np.stack([g.reshape(H, W) for g in gens[n - 1]]).astype(np.uint8)
                out['%s/dice%d' % (pre, n)] = dices[n - 1].numpy()
                out['%s/written%d' % (pre, n)] = np.asarray(sorted(k for k in range(K) if path_of(k, n) in saved), np.int64)
                assert len(out['%s/written%d' % (pre, n)]) == sum(p.endswith('_net%d.%s' % (n, 'png' if form == 'breast' else 'nii.gz'))
                                                                   for p in saved)
                out['%s/plane%d' % (pre, n)] = np.stack([plane(k, n) for k in range(K)])
                out['%s/target%d' % (pre, n)] = np.stack([after[k][n] for k in range(K)]).astype(np.uint8)
            have = sorted(path_of(k, n) for k in range(K) for n in (1, 2)
                          if (os.path.exists(path_of(k, n)) if form == 'breast' else path_of(k, n) in sitk.volumes))
            out[pre + '/files'] = np.asarray([os.path.relpath(p, os.path.join(train_root, folder)) for p in have], dtype='U64')
    out[key + '/form'] = np.asarray(form)
    out[key + '/orig'] = orig
    out[key + '/labelled'] = np.asarray(labelled, np.int64)
    out[key + '/ids_a'] = np.asarray(ids_a, dtype='U40')
    out[key + '/ids_b'] = np.asarray(ids_b, dtype='U40')
    out[key + '/update_percent'] = np.asarray(update_percent, np.float64)
    out[key + '/warmup'] = np.asarray(warmup, np.int64)
    out[key + '/n_epochs'] = np.asarray(len(epochs), np.int64)
    out[key + '/ref_lines'] = np.asarray(lines, np.int64)


def main():
    out = {}
    # 0-based epochs 2, 24, 29: (epoch + 1) = 3 (warm-up: open), 25 (closed), 30 (every tenth: open)
    # (the shifts of the predicted rectangles are drawn; the first seed whose epochs all meet the boundary condition is taken)
    for key, form, up in (('breast12', 'breast', 0.25), ('kidney12', 'kidney', 0.4)):
        for seed in range(24, 224):
            try:
                tmp = {}
                scenario(tmp, key, form, 12, up, [2, 24, 29], 20, seed=seed)
            except AssertionError:
                continue
            out.update(tmp)
            out[key + '/seed'] = np.asarray(seed, np.int64)
            break
        else:
            raise RuntimeError('no seed gives clean selection boundaries for ' + key)
    scenario(out, 'breast3', 'breast', 3, 0.25, [2], 20, seed=5)
    scenario(out, 'kidney3', 'kidney', 3, 0.25, [2], 20, seed=5)
    out['scenarios'] = np.asarray(['breast12', 'kidney12', 'breast3', 'kidney3'])
    # what the fixture must show (checked here, on the reference's own output)
    for key, n_sel in (('breast12', 3), ('kidney12', 4)):
        e0 = lambda name: out['%s/e0/%s' % (key, name)]
        d1, d2 = e0('dice1'), e0('dice2')
        assert not np.isnan(d1).any() and not np.isnan(d2).any()
        assert d1[1] == 0.0 and 1 not in e0('written1') and 1 not in e0('written2'), 'empty / empty: 0.0, worst, not written'
        assert d2[2] == 0.0 and 2 not in e0('written2') and np.argsort(d2, kind='stable').tolist().index(2) < n_sel
        assert d1[3] == 0.0 and 3 in e0('written1') and 3 in e0('written2'), 'empty target, non-empty prediction: written'
        assert d1[4] == d1[5] and d2[4] == d2[5]
        if key == 'breast12':
            assert d1[0] == 0.0 and 0 not in e0('written1'), 'the labelled image: inside the worst quarter, skipped'
        assert int(out[key + '/e1/logged']) == 0 and len(out[key + '/e1/written1']) == 0
        assert int(out[key + '/e0/logged']) == 2 and len(out[key + '/e2/written1']) > 0
    k = 'kidney12'
    assert 6 in out[k + '/e0/written1'] and len(np.unique(out[k + '/e2/plane1'][6])) == 2 and out[k + '/e2/target1'][6].max() == 0
    assert out[k + '/e2/dice2'][6] == 0.0, 'a constant original mask: all-zero targets whatever the plane holds'
    assert out['breast12/e2/target1'][3].max() == 1, 'later targets are what earlier epochs wrote'
    for key in ('breast3', 'kidney3'):
        assert len(out[key + '/e0/files']) == 0 and int(out[key + '/e0/logged']) == 2
    np.savez_compressed(OUT, **out)
    print('wrote %s (%d bytes)' % (OUT, os.path.getsize(OUT)))
    for key in ('breast12', 'kidney12'):
        for j in range(3):
            print(key, 'epoch', int(out['%s/e%d/epoch' % (key, j)]) + 1, 'written',
                  out['%s/e%d/written1' % (key, j)].tolist(), out['%s/e%d/written2' % (key, j)].tolist())


if __name__ == '__main__':
    torch.set_num_threads(1)
    main()
