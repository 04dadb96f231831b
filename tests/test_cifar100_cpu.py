"""CIFAR-100 plumbing on the CPU: the binary release's reader and the --dataset option."""
import json
import os
import runpy
import sys

import numpy as np
import torch

from distributed_pytorch_amd.data import get_datasets, load_cifar100


def test_binary_release_is_read_with_fine_labels(tmp_path):
    rng = np.random.default_rng(0)
    n = 5
    rec = rng.integers(0, 256, size=(n, 3074), dtype=np.uint8)
    rec[:, 0] = [3, 1, 19, 0, 7]  # coarse
    rec[:, 1] = [0, 99, 42, 17, 99]  # fine
    d = tmp_path / "cifar-100-binary"
    d.mkdir()
    rec.tofile(str(d / "train.bin"))
    rec[:2].tofile(str(d / "test.bin"))
    ds = load_cifar100(str(tmp_path), True)
    assert ds.labels.tolist() == [0, 99, 42, 17, 99] and ds.labels.dtype == torch.int64
    chw = rec[:, 2:].reshape(n, 3, 32, 32)
    assert ds.images.shape == (n, 32, 32, 3) and np.array_equal(ds.images.numpy(), chw.transpose(0, 2, 3, 1))
    train, test = get_datasets(str(tmp_path), False, dataset="cifar100")
    assert len(train) == n and len(test) == 2 and test.labels.tolist() == [0, 99]
    # no files: synthetic data with the dataset's class count
    syn, _ = get_datasets(str(tmp_path / "nope"), False, 256, 8, dataset="cifar100")
    assert syn.name == "synthetic" and 10 < int(syn.labels.max()) < 100


def test_cli_dataset_cifar100(tmp_path):
    """main.py --dataset cifar100 --synthetic trains on the CPU and reports 100 classes."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    jm = str(tmp_path / "m.json")
    argv = sys.argv
    sys.argv = ["main.py", "--device", "cpu", "--dataset", "cifar100", "--synthetic", "--batch-size", "4",
                "--max-iters", "2", "--train-size", "64", "--test-size", "8", "--json-metrics", jm]
    try:
        runpy.run_path(os.path.join(root, "main.py"), run_name="__main__")
    finally:
        sys.argv = argv
    rec = json.loads(open(jm).read().splitlines()[-1])
    assert rec["num_classes"] == 100 and rec["dataset"] == "cifar100"
    assert rec["iters_run"] == 2 and rec["test_loss"] == rec["test_loss"] and rec["test_loss"] > 0
