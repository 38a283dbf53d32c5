"""``RIDES['trunk_bwd']`` (torch_scae_amd/step_plan.py, ops._TrunkBackwardOffer):
the plan's side of the trunk's backward riding in the output attention's
backward launch, on stand-ins -- no device."""
import re

import pytest
import torch

from torch_scae_amd import ops, step_plan
from torch_scae_amd.step_plan import RIDES, StepPlan


def test_the_row_follows_the_tables_rules():
    ride = RIDES["trunk_bwd"]
    assert ride.scope == "offer"
    assert ride.carriers == ("_SeedAttention.backward",)
    assert ride.abi == "scae_object_encoder_bwd_gemm_f32"
    assert ride.readers == ()
    for node in ride.carriers:
        assert re.fullmatch(r"_[A-Za-z0-9]+\.(forward|backward)", node), node
        cls, meth = node.split(".")
        assert hasattr(getattr(ops, cls), meth), node
    # an offer is made ahead of the carrier's launch, never parked
    with pytest.raises(AssertionError):
        StepPlan().park("trunk_bwd", object())
    # the scopes' flushes still start with what they started with
    assert [k for k, r in RIDES.items() if r.scope != "offer"][:2] == \
        ["class_probs", "combine"]
    assert StepPlan().carry_trunk_bwd is True


class _Node:
    """What ops._SetEncoder.forward leaves on its autograd context."""
    dims = (5, 24, 16, 144, 0, 3, 1)
    bf16 = False
    carried = None

    @property
    def saved_tensors(self):
        raise AssertionError("a declined offer touches nothing")


class _Lib:
    """Every shape passes the predicate; any launcher call is an error."""

    @staticmethod
    def scae_object_encoder_bwd_supported(*a):
        return 1

    def __getattr__(self, name):
        raise AssertionError("launched " + name)


def _offer():
    z = torch.zeros(5, 24, 16)
    node = _Node()
    return ops._TrunkBackwardOffer(node, z), node, z


def test_an_offer_nobody_claims_leaves_the_trunk_to_launch_alone():
    plan = StepPlan()
    offer, node, z = _offer()
    with plan.fusing("image"):
        plan.offer("trunk_bwd", offer)
        assert plan.offers["trunk_bwd"] is offer
        # (no output attention in the model: nobody claims)
    assert plan.offers == {}
    # ``_SetEncoder.backward`` launches unless a carrier left a result here
    assert node.carried is None
    assert plan.claim("trunk_bwd") is None


def test_a_claimed_offer_is_declined_unless_everything_agrees():
    offer, node, z = _offer()
    lib, gh = _Lib(), torch.zeros_like(z)
    plan = StepPlan()
    # outside a parking plan (no fusion target / no deferred sums)
    assert not offer.carry(plan, lib, z, (), 24, 256, None, gh)
    with plan.fusing("image"):
        assert not plan.parking
        assert not offer.carry(plan, lib, z, (), 24, 256, None, gh)
        with plan.deferring():
            assert plan.parking
            # the attention reads another tensor than the trunk's output
            other = torch.zeros_like(z)
            assert not offer.carry(plan, lib, other, (), 24, 256, None, gh)
            # ... or a view of it with other sizes
            assert not offer.carry(plan, lib, z.view(5, 16, 24), (), 24, 256,
                                   None, gh)
            # the switch
            plan.carry_trunk_bwd = False
            assert not offer.carry(plan, lib, z, (), 24, 256, None, gh)
            plan.carry_trunk_bwd = True
            # the two nodes disagree about the precision
            with plan.precision(True):
                assert not offer.carry(plan, lib, z, (), 24, 256, None, gh)
            # everything agrees: the saved tensors are read for the launch
            with pytest.raises(AssertionError, match="touches nothing"):
                offer.carry(plan, lib, z, (), 24, 256, None, gh)
    assert node.carried is None


def test_fusing_clears_a_stale_offer():
    plan = StepPlan()
    offer, _, _ = _offer()
    plan.offers["trunk_bwd"] = offer        # (left by a step that raised)
    with plan.fusing("image"):
        assert plan.offers == {}
        plan.offer("trunk_bwd", offer)
    assert plan.offers == {}
    # a claim takes the offer out of the plan
    plan.offer("trunk_bwd", offer)
    assert plan.claim("trunk_bwd") is offer and plan.offers == {}
    # ... and plans do not share offers
    a, b = StepPlan("a"), StepPlan("b")
    a.offer("trunk_bwd", offer)
    assert b.claim("trunk_bwd") is None and a.claim("trunk_bwd") is offer
    assert step_plan.ambient.carry_trunk_bwd is True
