"""RandAugment + Cutout on the GPU: the LDS-resident policy kernel (augment_policy.hip) against the
integer CPU oracle (cpu_ref.augment_policy), bit for bit in the images and the targets."""
import pytest
import torch

from distributed_pytorch_amd.ops import cpu_ref

pytestmark = pytest.mark.gpu

MEAN, STD = [0.49, 0.48, 0.45], [0.25, 0.24, 0.26]
_SETS, _TABLES = {}, {}


def _C():
    from distributed_pytorch_amd import _ext

    return _ext.require()


def _image_set(Hs, Ws):
    """50 uint8 images, built once per shape: 48 random, one constant (all 0: one histogram bin whatever
    the crop pads) and one with a single non-empty bin per channel (two once the crop pads)."""
    if (Hs, Ws) not in _SETS:
        g = torch.Generator().manual_seed(5 + Hs)
        imgs = torch.randint(0, 256, (50, Hs, Ws, 3), dtype=torch.uint8, generator=g)
        imgs[48] = 0
        imgs[49] = torch.tensor([7, 200, 90], dtype=torch.uint8)
        labels = torch.randint(0, 10, (50,), generator=g)
        _SETS[(Hs, Ws)] = (imgs, labels, imgs.cuda(), labels.cuda())
    return _SETS[(Hs, Ws)]


def _table(M, Hs, Ws):
    if (M, Hs, Ws) not in _TABLES:
        t = cpu_ref.policy_params(M, Hs, Ws)
        _TABLES[(M, Hs, Ws)] = (t, t.cuda())
    return _TABLES[(M, Hs, Ws)]


def _idx(B):
    """B dataset indices: random images, then the constant one (B > 2) and the one-bin one."""
    idx = torch.randint(0, 48, (B,), generator=torch.Generator().manual_seed(B))
    idx[-1] = 49
    if B > 2:
        idx[-2] = 48
    return idx


def _both(Hs, Ws, pad, B, M, n_ops, cutout, force_op=-1, seed=99, salt=12345):
    """(oracle image, GPU image, the oracle's draws); asserts the targets equal."""
    imgs, labels, imgs_d, labels_d = _image_set(Hs, Ws)
    idx = _idx(B)
    tab, tab_d = _table(M, Hs, Ws)
    ref, rt = torch.empty(B, Hs, Ws, 4), torch.empty(B, dtype=torch.int64)
    draws = cpu_ref.augment_policy(imgs, idx, labels, ref, rt, pad, seed, salt, MEAN, STD, tab, n_ops, cutout, force_op)
    out = torch.full((B, Hs, Ws, 4), 7.0, device="cuda")
    t = torch.full((B,), -1, dtype=torch.int64, device="cuda")
    _C().augment_policy(imgs_d, idx.cuda(), labels_d, out, t, pad, seed, salt, MEAN, STD, tab_d, n_ops, cutout,
                        force_op)
    torch.cuda.synchronize()
    assert torch.equal(t.cpu(), rt)
    return ref, out, draws


@pytest.mark.parametrize("Hs,Ws,pad,B", [(32, 32, 4, 5), (6, 10, 2, 3), (64, 64, 4, 2)])
@pytest.mark.parametrize("op", range(14))
def test_each_op_alone_is_bitwise_the_oracle(op, Hs, Ws, pad, B):
    for M in (0, 9, 30):
        ref, out, _ = _both(Hs, Ws, pad, B, M, 2, 0, force_op=op)
        bad = (out.cpu() != ref).sum().item()
        assert bad == 0, f"{cpu_ref.POLICY_OPS[op]} M={M}: {bad} values differ"


@pytest.mark.parametrize("cutout", [0, 16])
@pytest.mark.parametrize("n_ops", [1, 2, 4])
def test_drawn_policy_is_bitwise_the_oracle(n_ops, cutout):
    for salt in (12345, 777):
        ref, out, draws = _both(32, 32, 4, 64, 9, n_ops, cutout, salt=salt)
        assert len({op for ops, _ in draws for op, _ in ops}) >= 10  # not an all-Identity batch
        assert len({sg for ops, _ in draws for _, sg in ops}) == 2
        assert torch.equal(out.cpu(), ref), f"salt {salt}"


def test_anchors_to_the_plain_augmentation():
    """No ops, no Cutout: bitwise augment(train=1).  Cutout alone: every pixel is the plain value or
    0.0 in all four channels, and the zero set is exactly the oracle's box."""
    Hs = Ws = 32
    B = 64
    imgs, labels, imgs_d, labels_d = _image_set(Hs, Ws)
    ref, out, _ = _both(Hs, Ws, 4, B, 9, 0, 0)
    idx = _idx(B)
    plain = torch.empty(B, Hs, Ws, 4, device="cuda")
    _C().augment(imgs_d, idx.cuda(), labels_d, plain, None, 4, True, 99, 12345, MEAN, STD)
    assert torch.equal(out, plain) and torch.equal(out.cpu(), ref)
    ref, out, draws = _both(Hs, Ws, 4, B, 9, 0, 16)
    box = torch.zeros(B, Hs, Ws, dtype=torch.bool)
    for b, (_, (y0, y1, x0, x1)) in enumerate(draws):
        box[b, y0:y1, x0:x1] = True
    assert 0 < box.sum().item() < B * Hs * Ws and len({d[1] for d in draws}) > B // 2
    box = box.cuda()
    assert torch.equal(out[~box], plain[~box])
    assert torch.equal(out[box], torch.zeros_like(out[box]))
    assert not (plain[~box][:, :3] == 0).all(1).any()  # outside the box nothing is zero by accident


def test_refusals_before_a_launch():
    imgs, labels, imgs_d, labels_d = _image_set(6, 10)
    idx = torch.arange(3).cuda()
    tab = _table(9, 6, 10)[1]
    o = lambda h=6, w=10: torch.empty(3, h, w, 4, device="cuda")
    run = lambda im, out, **kw: _C().augment_policy(
        im, idx, labels_d, out, None, 2, 1, 2, MEAN, STD, kw.get("table", tab), kw.get("n_ops", 2),
        kw.get("cutout", 0), kw.get("force_op", -1))
    run(imgs_d, o())  # the accepted call
    big = torch.zeros(3, 64, 65, 3, dtype=torch.uint8, device="cuda")
    for im, out, kw in ((big, o(64, 65), {}), (imgs_d, o(), {"n_ops": 5}), (imgs_d, o(), {"n_ops": -1}),
                        (imgs_d, o(), {"cutout": 7}), (imgs_d, o(), {"cutout": -1}), (imgs_d, o(), {"force_op": 14}),
                        (imgs_d, o(), {"force_op": -2}), (imgs_d, o(), {"table": tab[:60]}),
                        (imgs_d, o(), {"table": tab.float()})):
        with pytest.raises(RuntimeError):
            run(im, out, **kw)
    torch.cuda.synchronize()
    for M in (31, -1, 9.0):
        with pytest.raises(ValueError):
            cpu_ref.policy_params(M, 6, 10)
    with pytest.raises(ValueError):
        cpu_ref.policy_params(9, 64, 65)
