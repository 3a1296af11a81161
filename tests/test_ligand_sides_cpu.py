"""physdock_amd._ligand_sides: the host checks and the argmin that bestfit.BestFitRmsd and torsions.TorsionFingerprint share - the
messages each class gave before it shared them, word for word, and the nearest-target rule.  No GPU needed."""
import numpy as np
import pytest
import torch

from physdock_amd import _ligand_sides as sides
from physdock_amd import bestfit, torsions


def message(fn, *a, **k):
    with pytest.raises(ValueError) as e:
        fn(*a, **k)
    return str(e.value)


def test_each_class_keeps_its_messages():
    x = torch.zeros(2, 5, 3)
    idx = np.array([0, 1, 7], dtype=np.int64)
    for who, name, kernels in ((bestfit._WHO, "BestFitRmsd", "the kernel takes"), (torsions._WHO, "TorsionFingerprint", "the kernels take")):
        assert message(sides.host_idx, torch.zeros(3), "ligand_idx", name) == f"{name}: ligand_idx must hold integer atom indices, got torch.float32"
        assert message(sides.host_idx, [], "target_idx", name) == f"{name}: target_idx must be a non-empty 1-D list of integer atom indices"
        assert message(sides.host_idx, [1, -1], "target_idx", name) == f"{name}: target_idx holds a negative index"
        assert message(sides.structures, x[0], "x", None, 5, **who) == f"{name}: x must be a floating-point tensor [n,A,3], got (5, 3)"
        assert message(sides.structures, x[:0], "targets", None, 5, **who) == f"{name}: 0 structures in targets; {kernels} 1 .. 65535"
        assert message(sides.structures, x, "x", None, 4, **who) == f"{name}: x names 5 ligand atoms, expected 4"
        assert message(sides.structures, x, "x", idx, 3, **who) == f"{name}: an index of x (7) leaves its 5 atoms"
        assert message(sides.structures, x, "x", None, 5, **who) == f"{name}: x must be on the GPU, got a tensor on cpu"
        meta = torch.zeros(1, 5, 3, device="meta")
        assert message(sides.structures, meta, "targets", None, 5, device=torch.device("cpu"), **who) == \
            f"{name}: targets must be on the GPU of the poses, got a tensor on meta"
    # BestFitRmsd takes whatever a structure names (L None) up to its kernel's limit; TorsionFingerprint names its graph's atoms
    big = torch.zeros(1, bestfit.MAX_ATOMS + 1, 3)
    assert message(sides.structures, big, "x", None, None, **bestfit._WHO) == "BestFitRmsd: 1025 ligand atoms; the kernel takes 1 .. 1024"
    assert "max_atoms" not in torsions._WHO and bestfit.MAX_STRUCTURES == torsions.MAX_STRUCTURES == sides.MAX_STRUCTURES == 65535


def test_nearest_target():
    nan = float("nan")
    D = torch.tensor([[3.0, 1.0, 1.0, 2.0], [nan, nan, nan, nan], [nan, 5.0, nan, 4.0], [0.0, 0.0, 0.0, 0.0], [nan, 2.0, 2.0, nan]])
    near, value = sides.nearest(D)
    assert near.dtype == torch.int64 and value.dtype == torch.float32
    assert near.tolist() == [1, -1, 3, 0, 1]                       # the smallest index on a tie, -1 for an all-NaN row, a NaN never wins
    assert value[[0, 2, 3, 4]].tolist() == [1.0, 4.0, 0.0, 2.0] and bool(torch.isnan(value[1]))


def test_own_index_and_symmetry_flag():
    class Spec:
        ligand_idx = (4, 2, 9)

    class Cut:
        complete = False
    assert sides.own_idx(Spec).tolist() == [4, 2, 9] and sides.own_idx(Spec).dtype == np.int64
    Spec.ligand_idx = None
    assert sides.own_idx(Spec) is None
    assert sides.symmetry_complete(None) is True and sides.symmetry_complete(Cut) is False
    assert bestfit.BestFitRmsd([0, 1, 2]).symmetry_complete is True
