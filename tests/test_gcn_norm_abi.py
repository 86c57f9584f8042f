"""CPU checks of the normalised-GCN entries (added within ABI 22): the symbols
resolve, are bound and declared, the version stayed 22, every argument error
comes back as its negative code before anything touches a device, the Python
names exist with the stated signatures and refuse CPU tensors, the
constructor refuses what is out of scope, and ``GCNConv(8, 4)`` is still the
un-normalised layer."""
import inspect
import os
import re

import pytest
import torch

import ngnn
from ngnn import _lib, fused, ops

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "ngnn.h")
NAMES = ("ngnn_gcn_norm", "ngnn_gcn_wagg")
P = 256  # a dummy non-null, aligned pointer: a call that got past its checks would fault


def test_symbols_resolve_bound_and_declared_within_abi_22():
    lib = _lib.load()
    raw = open(HEADER).read()
    txt = re.sub(r"/\*.*?\*/", "", raw, flags=re.S)
    for name in NAMES:
        assert hasattr(lib, name), name
        assert name in _lib.SIGNATURES
        assert re.search(r"\b" + name + r"\s*\(", txt), name
    assert lib.ngnn_abi_version() == 22 and _lib.ABI_VERSION == 22
    assert int(re.search(r"#define NGNN_ABI_VERSION (\d+)", raw).group(1)) == 22
    block = raw[raw.index("symmetric-normalised GCN"):]
    assert "Added within ABI 22" in block
    # the header states the duplicate-self-loop rule and the rounding of dinv
    assert "LAST in CSR" in block and "no approximate reciprocal square root" in block


def _norm(lib, rowptr=P, col=P, w=P, n=300, loops=1, dinv=P, loop_w=P):
    return lib.ngnn_gcn_norm(rowptr, col, w, n, loops, dinv, loop_w, None)


def test_norm_argument_errors_return_before_launch():
    lib = _lib.load()
    assert _norm(lib, rowptr=None) == _lib.E_ARG
    assert _norm(lib, dinv=None) == _lib.E_ARG
    assert _norm(lib, loop_w=None) == _lib.E_ARG          # add_self_loops needs it
    assert _norm(lib, n=-1) == _lib.E_ARG
    assert _norm(lib, n=1 << 31) == _lib.E_RANGE
    assert _norm(lib, n=0) == _lib.OK                     # nothing to do, nothing read
    assert _norm(lib, n=0, col=None, w=None, loop_w=None) == _lib.OK


def _wagg(lib, z=P, ldz=47, F=47, rowptr=P, col=P, w=P, dinv=P, loop_w=P, bias=P, n=300, out=P, ldo=47):
    return lib.ngnn_gcn_wagg(z, ldz, F, rowptr, col, w, dinv, loop_w, bias, n, out, ldo, None)


def test_wagg_argument_errors_return_before_launch():
    lib = _lib.load()
    for name in ("z", "rowptr", "out"):
        assert _wagg(lib, **{name: None}) == _lib.E_ARG, name
    assert _wagg(lib, n=-1) == _lib.E_ARG
    assert _wagg(lib, F=-1) == _lib.E_ARG
    assert _wagg(lib, ldz=46) == _lib.E_SHAPE
    assert _wagg(lib, ldo=46) == _lib.E_SHAPE
    assert _wagg(lib, n=1 << 31) == _lib.E_RANGE
    assert _wagg(lib, F=1 << 31, ldz=1 << 31, ldo=1 << 31) == _lib.E_RANGE
    # no row or no column to write: success, nothing read (no pointer needed)
    assert _wagg(lib, n=0, z=None, out=None) == _lib.OK
    assert _wagg(lib, F=0, ldz=0, ldo=0, z=None, out=None) == _lib.OK


def test_python_names_signatures_and_cpu_refusal():
    sig = inspect.signature(ops.gcn_norm)
    assert list(sig.parameters) == ["block_or_edge_index", "edge_weight", "num_nodes", "add_self_loops"]
    assert [p.default for p in sig.parameters.values()][1:] == [None, None, True]
    sig = inspect.signature(ops.gcn_propagate)
    assert list(sig.parameters) == ["z", "block", "norm", "bias"] and sig.parameters["bias"].default is None
    sig = inspect.signature(ngnn.GCNConv.forward)
    assert list(sig.parameters) == ["self", "x", "edge_index", "edge_weight"]
    assert sig.parameters["edge_weight"].default is None
    sig = inspect.signature(ngnn.GCNConv.__init__)
    for k, d in (("normalize", False), ("add_self_loops", None), ("improved", False), ("cached", False)):
        assert sig.parameters[k].default == d or sig.parameters[k].default is d, k
    assert list(inspect.signature(ngnn.SimpleGCN.__init__).parameters)[-1] == "normalize"
    assert inspect.signature(ngnn.SimpleGCN.__init__).parameters["normalize"].default is False
    assert list(inspect.signature(ngnn.NGNN.__init__).parameters)[-1] == "gcn_normalize"
    assert inspect.signature(ngnn.NGNN.__init__).parameters["gcn_normalize"].default is False
    ei = torch.tensor([[0, 1], [1, 2]])
    with pytest.raises(RuntimeError):
        ops.gcn_norm(ei, num_nodes=3)
    with pytest.raises(RuntimeError):
        ngnn.GCNConv(4, 2, normalize=True)(torch.zeros(3, 4), ei)
    with pytest.raises(RuntimeError):
        ngnn.GCNConv(4, 2)(torch.zeros(3, 4), ei, torch.ones(2))


def test_constructor_refusals_and_defaults():
    with pytest.raises(NotImplementedError):
        ngnn.GCNConv(8, 4, normalize=True, improved=True)
    with pytest.raises(NotImplementedError):
        ngnn.GCNConv(8, 4, normalize=True, cached=True)
    with pytest.raises(NotImplementedError):
        ngnn.GCNConv(8, 4, normalize=False, add_self_loops=True)  # as before this feature
    with pytest.raises(NotImplementedError):
        ngnn.GCNConv(8, 4, bias=False)
    c = ngnn.GCNConv(8, 4)
    assert c.normalize is False and c.add_self_loops is False
    assert repr(c) == "GCNConv(8, 4)"
    assert not fused.weighted_gcn_layers(ngnn.SimpleGCN(8, 8, 4, 2))
    n = ngnn.GCNConv(8, 4, normalize=True)
    assert n.normalize and n.add_self_loops and "normalize=True" in repr(n)
    assert ngnn.GCNConv(8, 4, normalize=True, add_self_loops=False).add_self_loops is False
    assert sorted(n.state_dict()) == ["bias", "lin.weight"] == sorted(c.state_dict())
    m = ngnn.SimpleGCN(8, 8, 4, 3, normalize=True)
    assert fused.weighted_gcn_layers(m) == ["convs.0", "convs.1", "convs.2"]
    assert all(cv.normalize for cv in ngnn.NGNN(8, 8, 4, module="gcn", gcn_normalize=True).network.convs)
    assert not any(cv.normalize for cv in ngnn.NGNN(8, 8, 4, module="gcn").network.convs)


def test_bf16_is_refused_at_call_time_before_any_kernel():
    ei = torch.tensor([[0, 1], [1, 2]])
    x = torch.zeros(3, 4, dtype=torch.bfloat16)
    with pytest.raises(TypeError):  # bf16 parameters
        ngnn.GCNConv(4, 2, normalize=True).to(torch.bfloat16)(x.float(), ei)
    with pytest.raises(TypeError):  # bf16 input
        ngnn.GCNConv(4, 2, normalize=True)(x, ei)
    with pytest.raises(TypeError):  # the weighted un-normalised path too
        ngnn.GCNConv(4, 2)(x, ei, torch.ones(2))


def test_graph_capture_refuses_normalised_layers_by_name():
    from ngnn.graphs import GraphedTrainStep
    m = ngnn.SimpleGCN(8, 8, 4, 2, normalize=True)
    with pytest.raises(ValueError, match="convs.0"):
        GraphedTrainStep(m, torch.optim.Adam(m.parameters()), 4, 16, 64, 8, "cpu")
