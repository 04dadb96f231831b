"""RandAugment + Cutout without a GPU: the integer oracle (cpu_ref.policy_op / augment_policy)
against PIL where PIL is integer-defined, magnitude 0, the loader options and the command line."""
import argparse

import numpy as np
import pytest
import torch

from distributed_pytorch_amd.data import DeviceLoader
from distributed_pytorch_amd.data.cifar import synthetic_cifar
from distributed_pytorch_amd.ops import cpu_ref
from distributed_pytorch_amd.train import add_common_args, policy_args


def _image(seed=3, hw=32):
    return torch.randint(0, 256, (hw, hw, 3), dtype=torch.uint8, generator=torch.Generator().manual_seed(seed))


@pytest.mark.parametrize("M", [0, 9, 15, 30])
def test_posterize_solarize_equalize_are_pil(M):
    from PIL import Image, ImageOps

    img = _image()
    img[:, :, 2] = img[:, :, 2] // 3 + 100  # a channel with empty bins at both ends
    pil = Image.fromarray(img.numpy())
    tab = cpu_ref.policy_params(M, 32, 32)
    want = {10: ImageOps.posterize(pil, 8 - int(M / 7.5)), 11: ImageOps.solarize(pil, int(255 - 255 * M / 30)),
            13: ImageOps.equalize(pil)}
    for op, w in want.items():
        got = cpu_ref.policy_op(img.long(), op, 0, tab)
        assert torch.equal(got, torch.from_numpy(np.array(w)).long()), cpu_ref.POLICY_OPS[op]


def test_magnitude_zero_is_neutral_and_thirty_is_not():
    img = _image(4).long()
    zero, full = cpu_ref.policy_params(0, 32, 32), cpu_ref.policy_params(30, 32, 32)
    for op in cpu_ref.POLICY_SIGNED:
        for sign in (0, 1):
            assert torch.equal(cpu_ref.policy_op(img, op, sign, zero), img), cpu_ref.POLICY_OPS[op]
            out = cpu_ref.policy_op(img, op, sign, full)
            assert not torch.equal(out, img) and 0 <= out.min() and out.max() <= 255
        assert not torch.equal(cpu_ref.policy_op(img, op, 0, full), cpu_ref.policy_op(img, op, 1, full))


def test_loader_option_validation():
    ds = synthetic_cifar(24, seed=2)
    mk = lambda **kw: DeviceLoader(ds, 8, "cpu", seed=3, **kw)
    for kw in ({"randaugment": (2, 9), "mixup": 0.2}, {"cutout": 8, "cutmix": 1.0}, {"randaugment": (2, 9), "train": False},
               {"cutout": 8, "train": False}, {"randaugment": (5, 9)}, {"randaugment": (0, 9)}, {"randaugment": (2, 31)},
               {"randaugment": (2,)}, {"randaugment": (2, 9.5)}, {"cutout": 33}, {"cutout": -1}, {"cutout": 2.5}):
        with pytest.raises(ValueError):
            mk(**kw)
    assert mk().policy is None and mk(cutout=8).policy is not None


def test_loader_is_reproducible_and_resumes():
    ds = synthetic_cifar(40, seed=2)
    epochs = []
    for _ in range(2):
        loader = DeviceLoader(ds, 16, "cpu", seed=3, randaugment=(2, 9), cutout=16)
        loader.set_epoch(1)
        epochs.append([(x.clone(), t.clone()) for x, t in loader])
    assert [x.shape[0] for x, _ in epochs[0]] == [16, 16, 8]
    for (x0, t0), (x1, t1) in zip(*epochs):
        assert torch.equal(x0, x1) and torch.equal(t0, t1)
    tail = [(x.clone(), t.clone()) for x, t in loader.iterate(start_batch=1)]
    assert len(tail) == 2 and all(torch.equal(a, b) for p, q in zip(tail, epochs[0][1:]) for a, b in zip(p, q))
    plain = DeviceLoader(ds, 16, "cpu", seed=3)
    plain.set_epoch(1)
    x_plain = next(iter(plain))[0]
    assert not torch.equal(x_plain, epochs[0][0][0])  # the policy changed the batch
    assert (epochs[0][0][0] == 0).all(-1).any()       # and cut a box out of it


def _args(*argv):
    return add_common_args(argparse.ArgumentParser()).parse_args(list(argv))


def test_cli_parsing_and_validation():
    assert policy_args(_args()) == (None, 0)
    assert policy_args(_args("--randaugment", "2,9", "--cutout", "16")) == ((2, 9), 16)
    assert policy_args(argparse.Namespace()) == (None, 0)
    for argv in (("--randaugment", "2"), ("--randaugment", "2,x"), ("--randaugment", "5,9"), ("--randaugment", "2,31"),
                 ("--randaugment", "1,2,3"), ("--cutout", "33"), ("--cutout", "-1"),
                 ("--randaugment", "2,9", "--mixup", "0.2"), ("--cutout", "8", "--cutmix", "1.0")):
        with pytest.raises(ValueError):
            policy_args(_args(*argv))
