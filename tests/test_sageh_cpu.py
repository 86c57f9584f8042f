"""tests/sageh_ref.py (the CPU restatement of SAGEH the GPU tests compare
against) reproduces both fixtures made by the reference's own sageH.py
(tests/golden/make_golden_sageh.py) at rtol = atol = 1e-6: both outputs and
every weight gradient; and the host side of ngnn.SAGEH: state-dict keys, the
factory, what the constructors refuse."""
import os

import numpy as np
import pytest
import torch

import sageh_ref

CASES = {"sageh_block": dict(sizes=(100, 32, 47, 3)), "sageh_eval": dict(sizes=(8, 8, 3, 2))}
UNUSED = {"act.weight", "bnl.weight", "bnl.bias", "bnl.running_mean", "bnl.running_var", "bnl.num_batches_tracked"}


def load_case(golden_dir, name):
    rec = dict(np.load(os.path.join(golden_dir, name + ".npz")))
    state = {k[len("param/"):]: torch.as_tensor(v) for k, v in rec.items() if k.startswith("param/")}
    return rec, state


def conv_keys(L):
    return {f"convs.{i}.{p}" for i in range(L) for p in ("lin_l.weight", "lin_l.bias", "lin_r.weight")}


@pytest.mark.parametrize("name", sorted(CASES))
def test_restatement_reproduces_reference_fixture(golden_dir, name):
    rec, state = load_case(golden_dir, name)
    L = CASES[name]["sizes"][3]
    assert set(state) == conv_keys(L) | UNUSED
    assert {k[len("grad/"):] for k in rec if k.startswith("grad/")} == conv_keys(L)
    m = sageh_ref.SAGEH(*CASES[name]["sizes"], dropout=0.0)
    m.load_state_dict(state, strict=True)
    out, h = m(torch.as_tensor(rec["x"]), torch.as_tensor(rec["edge_index"]))
    torch.testing.assert_close(out.detach(), torch.as_tensor(rec["out/out"]), rtol=1e-6, atol=1e-6)
    torch.testing.assert_close(h.detach(), torch.as_tensor(rec["out/h"]), rtol=1e-6, atol=1e-6)
    assert bool((h >= 0).all()) and bool((h == 0).any()) and bool((h > 0).any())
    sageh_ref.fixture_loss(out, h, rec).backward()
    for k, p in m.named_parameters():
        if k in conv_keys(L):
            torch.testing.assert_close(p.grad, torch.as_tensor(rec["grad/" + k]), rtol=1e-6, atol=1e-6, msg=k)
        else:
            assert p.grad is None, k


def test_fixture_cases_are_what_they_say(golden_dir):
    assert bool(load_case(golden_dir, "sageh_block")[0]["meta/training"])
    assert not bool(load_case(golden_dir, "sageh_eval")[0]["meta/training"])


def test_keep_mask_is_applied_after_the_tap():
    torch.manual_seed(0)
    m = sageh_ref.SAGEH(6, 5, 3, 3)
    x = torch.randn(9, 6)
    ei = torch.randint(0, 9, (2, 30))
    keeps = [torch.rand(9, 5) < 0.5 for _ in range(2)]
    out, h = m(x, ei, keeps=keeps, scale=2.0)
    a = torch.relu(m.convs[0](x, ei)) * keeps[0] * 2.0
    h1 = torch.relu(m.convs[1](a, ei))
    torch.testing.assert_close(h, h1)
    torch.testing.assert_close(out, m.convs[2](h1 * keeps[1] * 2.0, ei))


# ---- the model's host side (no device needed)
def test_model_keys_match_the_reference_checkpoint(golden_dir):
    import ngnn
    _, state = load_case(golden_dir, "sageh_block")
    m = ngnn.SAGEH(100, 32, 47, 3)
    assert set(m.state_dict()) == set(state)
    m.load_state_dict(state, strict=True)
    assert torch.equal(m.convs[2].lin_r.weight.detach(), state["convs.2.lin_r.weight"])
    w = m.convs[0].lin_l.weight.detach().clone()
    act, bnw = m.act.weight.detach().clone(), m.bnl.weight.detach().clone()
    with torch.no_grad():
        m.bnl.weight.fill_(3.0)
    m.reset_parameters()  # the convs only
    assert torch.equal(m.act.weight.detach(), act) and bool((m.bnl.weight == 3.0).all()) and bnw.numel() == 128
    assert not torch.equal(m.convs[0].lin_l.weight.detach(), w)
    assert not hasattr(m, "inference")


def test_factory_and_constructor_limits():
    import ngnn
    f = ngnn.NGNN(in_size=24, hidden_size=16, out_size=5, num_layers=3, module="sageH", dropout=0.25)
    assert isinstance(f.network, ngnn.SAGEH) and len(f.network.convs) == 3 and f.network.dropout == 0.25
    held = {id(p) for grp in f.optimizer.param_groups for p in grp["params"]}
    assert {id(p) for p in f.network.parameters()} == held
    with pytest.raises(ValueError, match="num_layers"):
        ngnn.SAGEH(8, 8, 3, 1)
    with pytest.raises(ValueError):
        ngnn.NGNN(module="sageFC")
    pl = ngnn.NGNN(in_size=8, hidden_size=8, out_size=3, module="sagePL", nbr_nodes=5, sagepl_fused=True)
    assert pl.network.fused_stack is True
    assert ngnn.NGNN(in_size=8, hidden_size=8, out_size=3, module="sagePL", nbr_nodes=5).network.fused_stack is False
    assert ngnn.SAGEPL(8, 8, 3, 2, nbr_nodes=5).fused_stack is False
