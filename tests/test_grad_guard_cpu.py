"""Host side of the guarded optimizer step: the chunk table that drives ops.grad_guard against its restatement
(tests/grad_guard_ref.py), the Trainer's new keyword arguments, the declarations, and the optimizer's state dict."""
import os
import re

import numpy as np
import pytest
import torch

import grad_guard_ref as G

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("edm_grad_guard", "edm_adam_ema_guarded", "edm_adam_ema_phema_guarded")

# ragged layout: tensors at 64-element-aligned offsets (FlatArena's rule) with padding between them, one empty tensor
NUMELS = [1, 3, 64, 65, 0, 4097, 70001]


def _layout(numels=NUMELS):
    offs, pos = [], 0
    for c in numels:
        offs.append(pos)
        pos += (c + 63) // 64 * 64
    return offs, pos + 64


@pytest.mark.parametrize("chunk", [1024, 2048, 4096, 1 << 20])
def test_chunk_table_matches_the_reference_and_tiles_every_tensor_exactly(chunk):
    from tinyedm_amd import ops
    offs, n = _layout()
    numels = NUMELS
    ch, tn = ops.grad_guard_chunks(offs, numels, n, chunk)
    rch, rtn = G.chunk_table(offs, numels, n, chunk)
    assert ch.dtype == np.int64 and tn.dtype == np.int32
    assert [tuple(r) for r in ch.tolist()] == rch and [tuple(r) for r in tn.tolist()] == rtn
    covered = np.zeros(n, dtype=np.int32)
    owner = np.full(n, -1)
    for p, (o, c) in enumerate(zip(offs, numels)):
        owner[o:o + c] = p
    for t, first, length in ch.tolist():
        assert 1 <= length <= chunk
        covered[first:first + length] += 1
        assert (owner[first:first + length] == t).all(), "a chunk straddles two tensors or covers padding"
    assert ((covered == 1) == (owner >= 0)).all() and covered.max() == 1, "the chunks do not tile the tensors exactly"
    nb = 0
    for p, (first, cnt, b0, blocks) in enumerate(tn.tolist()):      # a tensor's chunks are consecutive, in element order
        assert (b0, blocks) == (nb, -(-numels[p] // ops.GUARD_BLOCK))   # ... and so are its partial-sum blocks
        nb += blocks
        rows = ch[first:first + cnt]
        assert (rows[:, 0] == p).all() and int(rows[:, 2].sum()) == numels[p]
        assert (rows[1:, 1] == rows[:-1, 1] + rows[:-1, 2]).all()
        if cnt:
            assert rows[0, 1] == offs[p] and (rows[:-1, 2] % ops.GUARD_BLOCK == 0).all()


def test_default_chunk_and_device_table_on_the_host():
    from tinyedm_amd import ops
    offs, n = _layout()
    tab = ops.grad_guard_table(offs, NUMELS, n, "cpu")
    ch, tn = ops.grad_guard_chunks(offs, NUMELS, n)
    assert tab.n == n and torch.equal(tab.chunks, torch.from_numpy(ch)) and torch.equal(tab.tensors, torch.from_numpy(tn))
    nb = int(tn[:, 3].sum())
    assert tab.part.shape == (nb,) and tab.part.dtype == torch.float64
    assert tab.flags.shape == (nb + len(NUMELS),) and tab.flags.dtype == torch.int32
    assert int(ch[:, 2].max()) == ops.GUARD_CHUNK and ops.GUARD_CHUNK % ops.GUARD_BLOCK == 0 and ops.GUARD_BLOCK == G.BLOCK


def test_table_rejects_overlapping_or_outlying_slices():
    """the slices ops.adam_ranges_table refuses (tests/test_fused_opt_gpu.py) are refused here too"""
    from tinyedm_amd import ops
    with pytest.raises(ValueError):
        ops.grad_guard_table([0, 5], [10, 10], 100, "cpu")
    with pytest.raises(ValueError):
        ops.grad_guard_table([95], [10], 100, "cpu")
    with pytest.raises(ValueError):
        ops.grad_guard_table([-4], [10], 100, "cpu")
    with pytest.raises(ValueError):
        ops.grad_guard_table([0, 16], [10], 100, "cpu")
    with pytest.raises(ValueError):
        ops.grad_guard_table([0], [0], 100, "cpu")
    with pytest.raises(ValueError):
        ops.grad_guard_table([0], [10], 100, "cpu", chunk=0)
    with pytest.raises(ValueError):
        ops.grad_guard_table([0], [10], 100, "cpu", chunk=1000)         # not a multiple of the 1024-element block
    for fn in (G.chunk_table,):
        with pytest.raises(ValueError):
            fn([0, 5], [10, 10], 100, 16)
        with pytest.raises(ValueError):
            fn([95], [10], 100, 16)


def test_reference_norm_and_coef():
    offs, n = _layout([3, 5])
    a = np.zeros(n, dtype=np.float32)
    a[0:3] = [3.0, 0.0, 4.0]
    a[64:69] = [1.0, 1.0, 1.0, 1.0, 0.0]
    a[10] = np.nan                                          # padding: belongs to no tensor
    per, total = G.sumsq(a, offs, [3, 5], 0.5)
    assert per.tolist() == [6.25, 1.0] and total == 7.25
    assert not G.nonfinite(a, offs, [3, 5], 0.5)
    a[68] = np.inf
    assert G.nonfinite(a, offs, [3, 5], 0.5)
    norm, c = G.coef(25.0, 1.0)
    assert norm == 5.0 and c == 1.0 / (5.0 + 1e-6)
    assert G.coef(25.0, 10.0) == (5.0, 1.0) and G.coef(25.0, None) == (5.0, 1.0) and G.coef(25.0, float("inf"))[1] == 1.0


def test_trainer_keyword_validation():
    import tinyedm_amd as T
    tr = T.Trainer()
    assert (tr.gradient_clip_val, tr.gradient_clip_algorithm, tr.skip_nonfinite_steps, tr.max_consecutive_skips) == \
        (None, "norm", False, 10)
    tr = T.Trainer(gradient_clip_val=1.0, gradient_clip_algorithm="value", skip_nonfinite_steps=True, max_consecutive_skips=3)
    assert (tr.gradient_clip_val, tr.gradient_clip_algorithm, tr.skip_nonfinite_steps, tr.max_consecutive_skips) == \
        (1.0, "value", True, 3)
    with pytest.raises(ValueError):
        T.Trainer(gradient_clip_val=-0.5)
    with pytest.raises(ValueError):
        T.Trainer(gradient_clip_val=float("nan"))
    with pytest.raises(ValueError):
        T.Trainer(gradient_clip_val=1.0, gradient_clip_algorithm="l1")
    with pytest.raises(ValueError):
        T.Trainer(skip_nonfinite_steps=True, max_consecutive_skips=0)
    T.Trainer(some_lightning_kwarg=3)                       # other unknown kwargs are still accepted and ignored


def test_trainer_refuses_clipping_with_another_optimizer():
    import tinyedm_amd as T
    from tinyedm_amd.ema import MisconfigurationException
    w = torch.nn.Parameter(torch.zeros(3))
    sgd = torch.optim.SGD([w], lr=0.1)
    for kw in (dict(gradient_clip_val=1.0), dict(skip_nonfinite_steps=True)):
        with pytest.raises(MisconfigurationException):
            T.Trainer(**kw)._set_guard(sgd)
    T.Trainer()._set_guard(sgd)                             # nothing asked for: any optimizer


def test_header_declares_the_entries_and_ops_binds_them():
    from tinyedm_amd import _lib, ops
    with open(os.path.join(ROOT, "include", "tinyedm_hip.h")) as f:
        header = f.read()
    with open(os.path.join(ROOT, "tinyedm_amd", "csrc", "grad_guard.hip")) as f:
        src = f.read()
    with open(os.path.join(ROOT, "tinyedm_amd", "csrc", "common.h")) as f:
        common = f.read()
    with open(os.path.join(ROOT, "tinyedm_amd", "ops.py")) as f:
        ops_src = f.read()
    for name in ENTRIES:
        assert re.search(r"\bint\s+" + name + r"\s*\(", header), name
        assert f'extern "C" int {name}(' in src and name in _lib.SIGNATURES and f'_lib.call("{name}"' in ops_src
        params = re.search(r"\bint\s+" + name + r"\s*\(([^)]*)\)", header).group(1)
        assert len(params.split(",")) == len(_lib.SIGNATURES[name]), name
    assert "edm_grad_guard_record" in header and "struct GuardRecord" in common
    assert ops.GUARD_RECORD.itemsize == 64
    assert [ops.GUARD_RECORD.fields[k][1] for k in ("coef", "skip", "norm", "clip_value", "sumsq", "steps", "skipped",
                                                     "clipped", "consecutive_skips")] == [0, 4, 8, 12, 16, 24, 32, 40, 48]
    assert "atomicAdd" not in src                           # fixed-order sums: no floating-point atomics
    # the unguarded kernels keep their text: the new ones live in a file of their own
    with open(os.path.join(ROOT, "tinyedm_amd", "csrc", "optim.hip")) as f:
        assert "guard" not in f.read().lower()


def test_ops_refuse_host_tensors_and_bad_limits():
    from tinyedm_amd import ops
    offs, n = _layout()
    tab = ops.grad_guard_table(offs, NUMELS, n, "cpu")
    with pytest.raises(RuntimeError):
        ops.grad_guard(torch.zeros(n), tab, torch.zeros(len(NUMELS), dtype=torch.float64), torch.zeros(8, dtype=torch.int64))
    with pytest.raises(ValueError):
        ops._guard_limit(-1.0, "max_norm")
    with pytest.raises(ValueError):
        ops._guard_limit(float("nan"), "clip_value")
    assert ops._guard_limit(None, "max_norm") == float("inf") and ops._guard_limit(0.5, "max_norm") == 0.5


def test_state_dict_has_no_guard_key_without_a_guard():
    from tinyedm_amd.ema import FusedAdam
    opt = FusedAdam([torch.nn.Parameter(torch.zeros(5)), torch.nn.Parameter(torch.zeros(2, 3))], lr=1e-3)
    assert opt.guard is None
    sd = opt.state_dict()
    assert "guard" not in sd
    assert set(sd) == {"m", "v", "step", "layout", "offsets", "numels", "param_groups"}
    assert opt.set_guard() is None and opt.guard is None and "guard" not in opt.state_dict()
    with pytest.raises(ValueError):
        opt.set_guard(max_norm=-1.0)
    with pytest.raises(RuntimeError):
        opt.guard_stats()


def test_yaml_overrides_reach_the_trainer():
    """experiments/train.py as it is: `trainer.gradient_clip_val=1.0 trainer.skip_nonfinite_steps=true` on the command line"""
    import tinyedm
    from tinyedm.config import compose
    conf = os.path.join(ROOT, "experiments", "conf")
    for name in ("cifar10",):
        plain = compose(name, conf, [])
        assert "gradient_clip_val" not in plain.trainer and "skip_nonfinite_steps" not in plain.trainer     # defaults unchanged
        cfg = compose(name, conf, ["trainer.gradient_clip_val=1.0", "trainer.skip_nonfinite_steps=true"])
        tr = tinyedm.Trainer(**{k: v for k, v in cfg.trainer.items()})
        assert tr.gradient_clip_val == 1.0 and tr.skip_nonfinite_steps is True and tr.gradient_clip_algorithm == "norm"
