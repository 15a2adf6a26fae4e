"""CPU: foreground masks of the SRN-format data -- make_synthetic_srn(masks=True)
writes them from the ray-caster's hit test, load_masks / SRN.masks read them."""
import os

import numpy as np
import torch

from codenerf_amd.data import SRN, load_imgs, load_masks, make_synthetic_srn


def _tree(base):
    return sorted(os.path.relpath(os.path.join(d, f), base) for d, _, fs in os.walk(base) for f in fs)


def test_synthetic_masks_agree_with_the_white_background(tmp_path):
    base = make_synthetic_srn(str(tmp_path), "srn_cars", "cars_test", n_obj=2, n_views=3, H=24, W=20, focal=24.6,
                              seed=5, masks=True)
    ds = SRN(cat="srn_cars", splits="cars_test", data_dir=str(tmp_path), n_test_views=3)
    assert len(ds) == 2
    for k, obj in enumerate(ds.ids):
        focal, H, W, imgs, poses = ds.return_test_val_data(obj)
        m = ds.masks(obj)
        assert m.shape == (3, 24, 20) and m.dtype == torch.float32
        assert set(m.unique().tolist()) == {0.0, 1.0}               # every view sees object and background
        assert torch.equal(m, (imgs < 1).any(-1).float())
        assert torch.equal(m, load_masks(os.path.join(base, obj, "mask"), np.arange(3)))
        assert ds[k][3].shape == imgs.shape                          # __getitem__ is unchanged


def test_default_writes_todays_tree(tmp_path):
    a = make_synthetic_srn(str(tmp_path / "a"), n_obj=1, n_views=2, H=16, W=16, focal=16.4, seed=2)
    b = make_synthetic_srn(str(tmp_path / "b"), n_obj=1, n_views=2, H=16, W=16, focal=16.4, seed=2, masks=True)
    assert not any(p.split(os.sep)[1] == "mask" for p in _tree(a))
    assert [p for p in _tree(b) if p.split(os.sep)[1] != "mask"] == _tree(a)
    for p in _tree(a):                                               # the masks change no other file
        assert open(os.path.join(a, p), "rb").read() == open(os.path.join(b, p), "rb").read(), p
    ds = SRN(cat="srn_cars", splits="cars_train", data_dir=str(tmp_path / "a"))
    assert ds.masks(ds.ids[0]) is None


def test_load_masks_round_trips(tmp_path):
    from PIL import Image
    g = torch.Generator().manual_seed(0)
    want = (torch.rand(4, 9, 7, generator=g) < 0.5).float()
    for i, m in enumerate(want):
        a = m.numpy().astype(np.uint8)
        # nonzero is foreground: 255, 1, and an RGB file with one nonzero channel
        if i == 2:
            a = np.stack([a * 0, a * 3, a * 0], -1)
        else:
            a = a * (255 if i % 2 == 0 else 1)
        Image.fromarray(a).save(str(tmp_path / f"{i:06d}.png"))
    got = load_masks(str(tmp_path), np.arange(4))
    assert got.dtype == torch.float32 and torch.equal(got, want)
    assert torch.equal(load_masks(str(tmp_path), [3, 1]), want[[3, 1]])
    assert load_imgs(str(tmp_path), [0]).shape == (1, 9, 7, 3)       # the same files, the image loader's naming
