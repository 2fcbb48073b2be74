"""The pin of the oracle: the REFERENCE'S OWN model code (its nets/ package, imported unchanged through the dependency
stand-ins of oracle/refshim) executed on CPU in fp64, as recorded in tests/golden/reference_pin.npz by
`tests/golden/make_reference_golden.py --pin`, and compared with

  * every golden fixture of tests/golden/*.npz (which tests/golden/make_reference_golden.py --write produced from it),
  * the oracle restatement oracle/nets.py built with the same weights (copied BY NAME, both directions checked),
  * the product's host mirror equiformer_amd.nets: every registered factory name, every parameter name / shape and --
    under the same torch seed -- every INITIAL VALUE, bit for bit (registry, names, init coupling; the pin
    holds a sha256 digest of the reference's initial values).

The full-width cases build the PRODUCT's model under the reference's seed, check that its initial values are the
reference's (digest), and copy them into the oracle, whose fp64 outputs must equal the reference's recorded ones; the two
OC20 cases ran the reference with the oracle's name-filled weights (tests/golden/weights.py), which the test fills again."""
import os
import sys
import warnings

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "golden"))
sys.path.insert(0, os.path.dirname(HERE))
import make_reference_golden as mrg  # noqa: E402

warnings.filterwarnings("ignore", category=FutureWarning)


@pytest.fixture(scope="module")
def pin():
    return mrg.load_pin()


def test_fixtures_and_oracle_equal_the_reference_model_code():
    errs = mrg.check_pinned(log=lambda *a: None)
    assert len({t for t, _ in errs}) == 10  # every fixture family
    bad = {k: v for k, v in errs.items() if max(v) > mrg.TOL}
    assert not bad, bad


def test_registry_names_parameters_and_initial_values_equal_the_reference(pin):
    from equiformer_amd import nets as pnets
    from equiformer_amd.nets import registry as preg
    ref_names = list(pin["reg::names"])
    assert len(ref_names) == 20
    assert set(ref_names) <= set(preg.list_models())
    for name in ref_names:
        torch.manual_seed(7)
        p = pnets.model_entrypoint(name)(**mrg.factory_kwargs(name))
        rt, pt = list(pin["reg::%s::params" % name]), list(mrg.param_table(p))
        rn, pn = [e.split(":")[0] for e in rt], [e.split(":")[0] for e in pt]
        assert set(rn) == set(pn), (name, sorted(set(rn) ^ set(pn))[:6])
        assert rn == pn, name  # registration ORDER too: optimizer checkpoints index parameters by position
        assert rt == pt, (name, [(a, b) for a, b in zip(rt, pt) if a != b][:6])  # shapes
        if name == "equiformer_md17_dens":
            # the product builds this model on top of its MD17 class, so force_embed draws its random numbers later
            # than in the reference (:134): same names / shapes / order, another RNG stream
            continue
        assert mrg.param_digest(p) == str(pin["reg::%s::digest" % name]), name  # every initial value, bit for bit
        assert sorted(p.no_weight_decay()) == list(pin["reg::%s::no_wd" % name]), name


@pytest.mark.parametrize("name,count", list(mrg.FULL_SIZE))
def test_full_size_baseline_factories_oracle_equals_reference(pin, name, count):
    """BASELINE configs at full width through the registry; the reference's own random initialisation (= the product's
    under the same seed, digest-checked) is copied into the oracle; fp64 forward (and forces) on a small batch."""
    from equiformer_amd import nets as pnets
    from oracle import nets as onets
    kw = mrg.factory_kwargs(name)
    torch.manual_seed(3)
    p = pnets.model_entrypoint(name)(**kw)
    assert int(pin["full::%s::count" % name]) == count  # SURVEY KAT-4 (the paper's parameter counts)
    assert sum(q.numel() for q in p.parameters()) == count
    assert mrg.param_digest(p) == str(pin["full::%s::digest" % name])
    o = onets.model_entrypoint(name)(**kw)
    mrg.copy_by_name(p, o)
    got = mrg.run_full_size(o.double().eval(), name)
    if "md17" in name:
        assert mrg.rel(got["forces"], pin["full::%s::forces" % name]) < 1e-9
    assert mrg.rel(got["energy"], pin["full::%s::energy" % name]) < 1e-10


def test_oc20_full_width_on_the_fly_periodic_graph_oracle_equals_reference(pin):
    """Config #5 (l1_256_nonlinear) through the reference's class with otf_graph=True / use_pbc=True: the reference's
    _forward_otf_graph + _forward_use_pbc (..._oc20.py:267-302) drove the periodic search; the oracle gets the edges and
    Cartesian offsets they produced (recorded in the pin).  Both ran with the same name-filled weights."""
    from oracle import pbc
    o = mrg.otf_oracle().double().eval()
    data = mrg.otf_input()
    t = torch.as_tensor
    ei, dist, off = pbc.get_pbc_distances(data.pos, t(pin["otf::edge_index"]), data.cell, t(pin["otf::cell_offsets"]),
                                          t(pin["otf::neighbors"]))
    assert ei.shape[1] > 100
    eo = o(data.atomic_numbers, data.tags, data.pos, data.batch, edge_index=ei, offsets=off)
    assert mrg.rel(eo.detach(), pin["otf::energy"]) < 1e-10


def test_oc20_e3_auxiliary_head_emits_1o_like_the_reference(pin):
    """E(3) feature with 1o channels + use_auxiliary_task: the head's output irreps are 1x1o [ref: ..._oc20.py:184-186]
    (the oracle and the product had 1x1e hard-coded until round 3)."""
    from equiformer_amd.nets.graph_attention_transformer_oc20 import GraphAttentionTransformerOC20 as ProdOC20
    # the product builds it too since round 4 (values against the oracle on the GPU: tests/test_gpu_oc20_heads.py): same
    # parameter names, shapes and order as the reference
    prod = ProdOC20(None, None, 1, use_pbc=True, otf_graph=False, **mrg.AUX_CFG)
    assert list(mrg.param_table(prod)) == list(pin["aux::params"])
    o = mrg.aux_oracle()
    assert list(mrg.param_table(o)) == list(pin["aux::params"])
    o = o.double().eval()  # the weights the reference ran with (name-filled)
    ins, _ = mrg.load_fixture("oc20_aux_small")
    t = torch.as_tensor
    eo, ao = o(t(ins["z"]), t(ins["tags"]), t(ins["pos"]).double(), t(ins["batch"]), edge_index=t(ins["edge_index"]),
               offsets=t(ins["offsets"]).double())
    assert ao.shape[-1] == 3 and np.asarray(pin["aux::aux"]).shape == tuple(ao.shape)
    assert mrg.rel(eo.detach(), pin["aux::energy"]) < 1e-10 and mrg.rel(ao.detach(), pin["aux::aux"]) < 1e-10
