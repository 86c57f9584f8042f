"""tests/sagepl_ref.py (the CPU restatement of SAGEPL the GPU tests compare
against) reproduces both fixtures made by the reference's own sagePL.py
(tests/golden/make_golden_sagepl.py): six outputs, the n_id rows of the noise
table's gradient (every other row zero) and every weight gradient, at
rtol = atol = 1e-6."""
import os

import numpy as np
import pytest
import torch

import sagepl_ref

CASES = {"sagepl_block": dict(sizes=(100, 32, 47, 3)), "sagepl_sign": dict(sizes=(8, 8, 3, 2))}


def load_case(golden_dir, name):
    rec = dict(np.load(os.path.join(golden_dir, name + ".npz")))
    state = {k[len("param/"):]: torch.as_tensor(v) for k, v in rec.items() if k.startswith("param/")}
    n_id = torch.as_tensor(rec["n_id"]) if "n_id" in rec else None
    return rec, state, n_id


@pytest.mark.parametrize("name", sorted(CASES))
def test_restatement_reproduces_reference_fixture(golden_dir, name):
    rec, state, n_id = load_case(golden_dir, name)
    nbr_nodes = state["noise"].shape[0]
    m = sagepl_ref.SAGEPL(*CASES[name]["sizes"], nbr_nodes=nbr_nodes, dropout=0.0).eval()
    m.load_state_dict(state, strict=True)
    outs = m(torch.as_tensor(rec["x"]), torch.as_tensor(rec["edge_index"]),
             noise_rate=float(rec["noise_rate"]), n_id=n_id)
    for nm, o in zip(sagepl_ref.OUT_NAMES, outs):
        torch.testing.assert_close(o.detach(), torch.as_tensor(rec["out/" + nm]), rtol=1e-6, atol=1e-6, msg=nm)
    sagepl_ref.fixture_loss(outs, rec).backward()
    assert bool(rec["grad/noise_rest_zero"])
    rows = torch.arange(nbr_nodes) if n_id is None else n_id
    gn = m.noise.grad
    torch.testing.assert_close(gn[rows], torch.as_tensor(rec["grad/noise_rows"]), rtol=1e-6, atol=1e-6)
    rest = torch.ones(nbr_nodes, dtype=torch.bool)
    rest[rows] = False
    assert (gn[rest] == 0).all()
    for k, p in m.named_parameters():
        if k != "noise":
            torch.testing.assert_close(p.grad, torch.as_tensor(rec["grad/" + k]), rtol=1e-6, atol=1e-6, msg=k)


def test_block_fixture_holds_a_zero_noise_row(golden_dir):
    rec, state, n_id = load_case(golden_dir, "sagepl_block")
    z = int(rec["meta/zero_row"])
    assert z in n_id.tolist() and (state["noise"][z] == 0).all()
    # the clamped-norm gradient: g * rate / 1e-12, large and finite
    row = torch.as_tensor(rec["grad/noise_rows"])[n_id.tolist().index(z)]
    assert torch.isfinite(row).all() and float(row.abs().max()) > 1e6


def test_sign_fixture_holds_exact_zeros(golden_dir):
    rec, _, n_id = load_case(golden_dir, "sagepl_sign")
    assert n_id is None and (rec["x"] == 0).any() and (rec["x"] < 0).any()


# ---- the model's host side (no device needed)
def test_model_keys_match_the_reference_checkpoint(golden_dir):
    import ngnn
    _, state, _ = load_case(golden_dir, "sagepl_block")
    m = ngnn.SAGEPL(100, 32, 47, 3, nbr_nodes=250)
    assert set(m.state_dict()) == set(state)
    m.load_state_dict(state, strict=True)
    assert torch.equal(m.noise.detach(), state["noise"])
    w = m.convs[0].lin_l.weight.detach().clone()
    noise = m.noise.detach().clone()
    m.reset_parameters()  # the convs only
    assert torch.equal(m.noise.detach(), noise) and not torch.equal(m.convs[0].lin_l.weight.detach(), w)
    for meth in ("forward_pure", "forward_noisy", "adding_noise", "inference"):
        assert callable(getattr(m, meth))


def test_factory_and_constructor_limits():
    import ngnn
    f = ngnn.NGNN(in_size=24, hidden_size=16, out_size=5, num_layers=2, module="sagePL", nbr_nodes=30)
    assert isinstance(f.network, ngnn.SAGEPL) and tuple(f.network.noise.shape) == (30, 24)
    assert any(p is f.network.noise for grp in f.optimizer.param_groups for p in grp["params"])
    with pytest.raises(ValueError):
        ngnn.SAGEPL(8, 8, 3, 1, nbr_nodes=10)
    with pytest.raises(ValueError):
        ngnn.NGNN(module="sageFC")
    with pytest.raises(ValueError):  # GPU only: no CPU fallback
        ngnn.add_node_noise(torch.zeros(2, 4), torch.zeros(2, 4))
