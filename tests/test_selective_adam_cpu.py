"""Row-selective Adam without a GPU: the restatement the GPU tests compare with, the C entry's struct mirror
and argument validation (nothing is launched), and what optim.SelectiveAdam / the two training setups do on the host."""
import ctypes
import types

import numpy as np
import pytest
import torch

import selective_adam_ref as R

ARGS = types.SimpleNamespace(percent_dense=0.01, position_lr_init=0.00016, position_lr_final=0.0000016,
                             position_lr_delay_mult=0.01, position_lr_max_steps=30000, feature_lr=0.0025, opacity_lr=0.05,
                             scaling_lr=0.005, rotation_lr=0.001, semantic_feature_lr=0.001)


@pytest.fixture(scope="module")
def lib():
    import os
    from gags_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        _lib.build()
    return _lib.load()


def _arrays(n, w, seed):
    rng = np.random.default_rng(seed)
    f = lambda a: np.asarray(a, np.float32)  # noqa: E731
    return f(rng.standard_normal((n, w))), f(rng.standard_normal((n, w))), f(rng.standard_normal((n, w)) * 0.1), \
        f(rng.random((n, w)) * 0.01)


# ----------------------------------------------------------------------------------------------------------------------
# the restatement
# ----------------------------------------------------------------------------------------------------------------------
def test_no_bias_step_underflows_for_the_betas_used():
    assert R.no_bias_step_is_exact(0.9, 0.999) and R.no_bias_step_is_exact(0.5, 0.99) and R.no_bias_step_is_exact(0.0, 0.0)
    assert not R.no_bias_step_is_exact(0.9, 0.9999999)   # (a beta for which the restatement would NOT be the declared rule)


def test_all_true_is_the_oracle_and_all_false_is_the_input(oracle):
    p, g, m, v = _arrays(37, 5, seed=1)
    po, mo, vo = p.copy(), m.copy(), v.copy()
    oracle.adam_step(po, g, mo, vo, 1e-3, eps=1e-15, step=3)
    for mask in (np.ones(37, np.uint8), None):
        got = R.step(oracle, p, g, m, v, 1e-3, mask=mask, step=3)
        for a, b in zip(got, (po, mo, vo)):
            R.assert_same_bits(a, b)
    got = R.step(oracle, p, g, m, v, 1e-3, mask=np.zeros(37, bool), step=3)
    for a, b in zip(got, (p, m, v)):
        R.assert_same_bits(a, b)
    # a mask and the zero test together, and what counts as zero
    g[3] = 0.0
    g[4] = -0.0
    g[5] = 0.0
    g[5, -1] = np.nan
    g[6] = 0.0
    g[6, -1] = 1e-30
    assert R.nonzero_rows(g)[[3, 4, 5, 6]].tolist() == [False, False, True, True]
    mask = np.arange(37) % 2 == 0
    sel = R.selection(g, mask, True)
    assert sel[[3, 4, 5, 6, 7, 8]].tolist() == [False, False, False, True, False, True]
    got = R.step(oracle, p, g, m, v, 1e-3, mask=mask, skip_zero_rows=True, step=3)
    assert np.array_equal(got[0][~sel], p[~sel]) and np.array_equal(got[1][~sel], m[~sel]) and np.array_equal(got[2][~sel], v[~sel])
    assert not np.array_equal(got[1][sel], m[sel])


@pytest.mark.parametrize("g", [0.37, -2.5e-3, 41.0])
def test_first_step_closed_forms(oracle, g):
    """From zero moments, parameter 0, one row.  With bias correction the first step is lr g / (|g| + eps); without it,
    lr (1 - b1) g / (sqrt(1 - b2) |g| + eps).  Bound: the float32 chain has 13 roundings (three host scalars and bc2_sqrt
    rounded to float32, the products, the square root, two divisions, the sum with eps, the final product; the subtraction
    from 0 is exact), each at most 2^-24 relative: 16 x 2^-24 of the float64 value."""
    lr, b1, b2, eps = 1e-3, 0.9, 0.999, 1e-15
    z = np.zeros((1, 1), np.float32)
    gg = np.full((1, 1), g, np.float32)
    g64 = float(gg[0, 0])
    for bias, want in ((True, -lr * g64 / (abs(g64) + eps)),
                       (False, -lr * (1 - b1) * g64 / (np.sqrt(1 - b2) * abs(g64) + eps))):
        p, m, v = R.step(oracle, z, gg, z, z, lr, mask=np.ones(1, bool), bias_correction=bias, beta1=b1, beta2=b2, eps=eps, step=1)
        assert abs(float(p[0, 0]) - want) <= 16 * 2.0 ** -24 * abs(want), (bias, float(p[0, 0]), want)
        assert m[0, 0] == np.float32(1 - b1) * gg[0, 0] and v[0, 0] == (np.float32(1 - b2) * gg[0, 0]) * gg[0, 0]


# ----------------------------------------------------------------------------------------------------------------------
# the C entry: struct mirror and validation (GAGS_EINVAL before any launch)
# ----------------------------------------------------------------------------------------------------------------------
def test_struct_mirror_and_constants_agree_with_the_header(lib):
    import os
    import re
    from gags_amd import _lib
    assert lib.gags_adam_tensor_bytes() == ctypes.sizeof(_lib.AdamTensor) == 72
    src = open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "include", "gags_raster.h")).read()
    defs = {k: int(v) for k, v in re.findall(r"^#define\s+(GAGS_ADAM_\w+)\s+(\d+)\b", src, flags=re.M)}
    assert defs == {"GAGS_ADAM_MAX_TENSORS": 8, "GAGS_ADAM_SKIP_ZERO_ROWS": 1, "GAGS_ADAM_NO_BIAS_CORRECTION": 2}
    for name, value in defs.items():
        assert getattr(_lib, name) == value


def test_validation_returns_einval_without_launching(lib):
    from gags_amd import _lib
    buf = (ctypes.c_float * 64)()
    base = ctypes.addressof(buf)
    al = base + (-base % 16)
    P = ctypes.c_void_p

    def call(n_rows=4, n_tensors=1, flags=0, step=1, mask=None, table=True, **over):
        d = dict(param=al, grad=al + 16, exp_avg=al + 32, exp_avg_sq=al + 48, width=1, lr=1e-3, beta1=0.9, beta2=0.999, eps=1e-15)
        d.update(over)
        t = (_lib.AdamTensor * 9)(*[_lib.AdamTensor(**d) for _ in range(9)])
        return lib.gags_adam_step_rows(n_rows, n_tensors, ctypes.cast(t, P) if table else None, mask, flags, step, None)

    assert call(n_rows=0) == 0                          # the baseline of every line below: valid arguments, nothing to do
    assert call(n_rows=0, n_tensors=8, flags=3) == 0
    assert call(n_rows=0, param=al + 4, width=45) == 0  # 4-byte alignment is enough
    assert call(n_rows=-1) == -1
    assert call(n_rows=0, n_tensors=0) == -1 and call(n_rows=0, n_tensors=9) == -1 and call(n_rows=0, n_tensors=-1) == -1
    assert call(n_rows=0, step=0) == -1 and call(n_rows=0, step=-3) == -1
    assert call(n_rows=0, width=0) == -1 and call(n_rows=0, width=-4) == -1
    assert call(n_rows=0, beta1=1.0) == -1 and call(n_rows=0, beta1=-0.1) == -1 and call(n_rows=0, beta1=float("nan")) == -1
    assert call(n_rows=0, beta2=1.0) == -1 and call(n_rows=0, beta2=-0.1) == -1
    assert call(n_rows=0, eps=-1e-8) == -1 and call(n_rows=0, eps=float("nan")) == -1
    assert call(n_rows=0, flags=4) == -1 and call(n_rows=0, flags=-1) == -1
    assert call(n_rows=0, table=False) == -1
    for name in ("param", "grad", "exp_avg", "exp_avg_sq"):
        assert call(n_rows=0, **{name: al + 2}) == -1, name    # not 4-byte aligned
        assert call(n_rows=0, **{name: al + 1}) == -1, name
        assert call(n_rows=4, **{name: None}) == -1, name      # NULL with rows to update
        assert call(n_rows=0, **{name: None}) == 0, name
    # the rule is checked for EVERY tensor of the table, not the first
    t = (_lib.AdamTensor * 2)(_lib.AdamTensor(al, al, al, al, 4, 1e-3, 0.9, 0.999, 1e-15),
                              _lib.AdamTensor(al, al, al, al, 0, 1e-3, 0.9, 0.999, 1e-15))
    assert lib.gags_adam_step_rows(0, 1, ctypes.cast(t, P), None, 0, 1, None) == 0
    assert lib.gags_adam_step_rows(0, 2, ctypes.cast(t, P), None, 0, 1, None) == -1


# ----------------------------------------------------------------------------------------------------------------------
# optim.SelectiveAdam and the training setups on the host
# ----------------------------------------------------------------------------------------------------------------------
def _cpu_model(n=12, d=16):
    from gags_amd.scene import GaussianModel
    g = torch.Generator().manual_seed(0)
    r = lambda *s: torch.randn(*s, generator=g)  # noqa: E731
    return GaussianModel.from_tensors(r(n, 3), r(n, 3), r(n, 4), r(n, 1), r(n, 1, 3), r(n, 3, 3), r(n, d), sh_degree=1)


def test_selective_adam_constructor_and_cpu_tensors():
    from gags_amd.optim import FeatureAdam, SelectiveAdam
    p = torch.nn.Parameter(torch.zeros(5, 4))
    opt = SelectiveAdam([{"params": [p], "lr": 1e-3, "name": "x"}], lr=0.0, eps=1e-15)
    assert isinstance(opt, FeatureAdam) and opt.skip_zero_rows is False and opt.bias_correction is True
    opt.step()                                           # no gradient: nothing to do, as FeatureAdam
    p.grad = torch.ones(5, 4)
    with pytest.raises(RuntimeError, match="no CPU path"):
        opt.step()
    with pytest.raises(RuntimeError, match="no CPU path"):
        opt.step(torch.ones(5, dtype=torch.bool))
    opt.zero_grad(set_to_none=True)
    assert p.grad is None
    opt = SelectiveAdam([p], lr=1e-3, skip_zero_rows=True, bias_correction=False)
    assert opt.skip_zero_rows is True and opt.bias_correction is False
    with pytest.raises(NotImplementedError):
        SelectiveAdam([p], weight_decay=0.1)
    with pytest.raises(NotImplementedError):
        SelectiveAdam([p], amsgrad=True)
    for bad in (dict(lr=-1.0), dict(eps=-1.0), dict(betas=(1.0, 0.999)), dict(betas=(0.9, -0.1))):
        with pytest.raises(ValueError):
            SelectiveAdam([p], **bad)


def test_checkpoints_are_interchangeable_with_feature_adam():
    """The two options are attributes of the optimizer, not of its groups: a state_dict of one class loads into the other."""
    from gags_amd.optim import FeatureAdam, SelectiveAdam
    def make(cls, **kw):
        p = torch.nn.Parameter(torch.zeros(5, 4))
        opt = cls([{"params": [p], "lr": 2e-3, "name": "x"}], lr=0.0, eps=1e-15, **kw)
        return p, opt
    p, sel = make(SelectiveAdam, skip_zero_rows=True)
    sel.state[p] = {"step": torch.tensor(7.0), "exp_avg": torch.full((5, 4), 0.5), "exp_avg_sq": torch.full((5, 4), 0.25)}
    q, dense = make(FeatureAdam)
    assert sel.state_dict()["param_groups"] == dense.state_dict()["param_groups"]
    dense.load_state_dict(sel.state_dict())
    assert float(dense.state[q]["step"]) == 7.0 and torch.equal(dense.state[q]["exp_avg"], sel.state[p]["exp_avg"])
    p2, sel2 = make(SelectiveAdam)
    sel2.load_state_dict(dense.state_dict())
    assert float(sel2.state[p2]["step"]) == 7.0 and torch.equal(sel2.state[p2]["exp_avg_sq"], sel.state[p]["exp_avg_sq"])
    assert sel2.skip_zero_rows is False


def test_training_setups_take_an_optimizer_type():
    from gags_amd.optim import FeatureAdam, SelectiveAdam
    m = _cpu_model()
    with pytest.raises(ValueError, match="optimizer_type"):
        m.training_setup(optimizer_type="nope")
    with pytest.raises(ValueError, match="optimizer_type"):
        m.training_setup_rgb(ARGS, optimizer_type="nope")
    opt = m.training_setup(optimizer_type="default")
    assert type(opt) is torch.optim.Adam and type(m.training_setup()) is torch.optim.Adam
    opt = m.training_setup(0.002, optimizer_type="sparse_adam")
    assert type(opt) is SelectiveAdam and opt.skip_zero_rows and opt.bias_correction
    assert [g["name"] for g in opt.param_groups] == ["semantic_feature"] and opt.param_groups[0]["lr"] == 0.002
    assert opt.param_groups[0]["eps"] == 1e-15 and opt.param_groups[0]["params"][0] is m._semantic_feature
    assert not isinstance(torch.optim.Adam([m._semantic_feature]), FeatureAdam)
