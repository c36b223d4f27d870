"""Networks whose nodes have five to eight parents, for the item kernels (bn_small.hip, bn_mid.hip, bn_maxprod.hip, bn_em.hip): the one
entry routine they all call (item_entry, bn_small_dev.hpp) runs a wave at its largest parent count, 5 and 6 in the MM = 6 instantiation and 7 and 8 in MM = 8, and a lane with
fewer parents loads element 0 of the pi-message array for each factor it lacks and multiplies by 1.0 instead.  Builders only, shared
by tests/test_many_parents_refs.py (the plans, on the CPU) and tests/test_many_parents_gpu.py (the kernels)."""
import numpy as np

from bayesiannetwork_amd import Evidence, from_parent_lists, synth
from test_em_gpu import _tables   # 0.1 + uniform, row-normalised


def _fan_lists(ms, kp, kc, first=0):
    """max(ms) roots of arity kp; one child of arity kc per m in ms over the first m roots; one arity-3 leaf below each child.
    Node numbers start at `first`."""
    roots = max(ms)
    k = [kp] * roots + [kc] * len(ms) + [3] * len(ms)
    parents = [[] for _ in range(roots)] + [[first + u for u in range(m)] for m in ms] + [[first + roots + c] for c in range(len(ms))]
    return k, parents


def fan(ms, kp=2, kc=2, seed=8):
    k, parents = _fan_lists(ms, kp, kc)
    return from_parent_lists(k, parents, _tables(k, parents, seed), name="fan" + "_".join(map(str, ms)) + f"_kp{kp}_kc{kc}")


def canary_fan(ms, kp=2, kc=2, seed=8):
    """fan(ms) behind a component of its own, node 0 (arity 3) -> node 1 (arity 2): edge 0 is that chain's, so element 0 of the
    pi-message array -- what a padded factor loads -- is the chain's to spoil (canary_evidence)."""
    fk, fpar = _fan_lists(ms, kp, kc, first=2)
    k, parents = [3, 2] + fk, [[], [0]] + fpar
    return from_parent_lists(k, parents, _tables(k, parents, seed), name="canary_fan" + "_".join(map(str, ms)))


def canary_evidence(model):
    """an all-zero vector on node 0: 0 / 0 = NaN in pi_msg[0:3] and in the beliefs of nodes 0 and 1, and nowhere else -- unless a
    padded factor lets the value it loaded through"""
    return Evidence.from_dict(model, {0: np.zeros(int(model.k[0]))})


CANARY_ELEMENTS = 3 + 2   # the belief elements of the canary's two nodes, in front of the fan's


def many_parent_child(model):
    """the first node with the largest parent count"""
    counts = np.diff(model.in_ptr)
    return int(np.argmax(counts))


def soft_zero(model):
    """a soft evidence vector with a zero in it on a many-parent child"""
    v = many_parent_child(model)
    w = 0.25 + np.arange(int(model.k[v]), dtype=float)
    w[0] = 0.0
    return Evidence.from_dict(model, {v: w})


# one-workgroup networks (tests/test_many_parents_refs.py pins what their plans hold)
SMALL = {
    "fan5": lambda: fan([5]),
    "fan6": lambda: fan([6]),
    "fan7": lambda: fan([7]),
    "fan8": lambda: fan([8]),
    "fan5_kp3": lambda: fan([5], kp=3),                              # a 486-entry table: 162-term runs
    "fan5_kp4": lambda: fan([5], kp=4),                              # 2 048 entries: three rounds, the kernels' four-round instantiation
    "fan7x6": lambda: fan([7] * 6),                                  # 1 586 entries on 12 waves: three rounds at 7 parents
    "fan5678": lambda: fan([5, 6, 7, 8]),                            # two rounds, every count in waves of its own
    "fan88": lambda: fan([8, 8]),
    "fan5_kc3": lambda: fan([5], kc=3),                              # 96 entries: the 5-parent node's second wave is shared with its leaf's
    "dag20_8parents": lambda: synth.random_dag(20, 8, 20, 2, seed=3),
    "dag26_8parents": lambda: synth.random_dag(26, 8, 26, 2, seed=5),
}
SMALL_PLAN = {   # name: (re, mmax, waves or None)
    "fan5": (1, 5, 4), "fan6": (1, 6, 4), "fan7": (1, 7, 5), "fan8": (1, 8, 9), "fan5_kp3": (1, 5, None), "fan5_kp4": (3, 5, 12),
    "fan7x6": (3, 7, 12), "fan5678": (2, 8, 12), "fan88": (2, 8, None), "fan5_kc3": (1, 5, None), "dag20_8parents": (2, 8, None),
    "dag26_8parents": (2, 7, None),
}
SMALL_CANARY = {"canary_fan5": lambda: canary_fan([5]), "canary_fan7": lambda: canary_fan([7]), "canary_fan5678": lambda: canary_fan([5, 6, 7, 8])}

# several-workgroup networks, and the number of parts of each plan
MID = {
    "fan8x4": lambda: fan([8] * 4),
    "dag40_8parents": lambda: synth.random_dag(40, 8, 20, 2, seed=3),
    "dag60_6parents_mixed": lambda: synth.random_dag(60, 6, 16, [2, 3, 2, 2, 3], seed=7),   # lanes of 0, 1, 3 and 5 parents in one wave
    "dag40_8parents_k223": lambda: synth.random_dag(40, 8, 20, [2, 2, 3], seed=5),          # parts of TWO rounds at 7 and at 8 parents
}
MID_PARTS = {"fan8x4": 6, "dag40_8parents": 17, "dag60_6parents_mixed": 22, "dag40_8parents_k223": 18}
MID_CANARY = {"canary_fan8x4": lambda: canary_fan([8] * 4),                       # (no lane pads at 8 parents: NaNs across parts only)
              "canary_fan575788": lambda: canary_fan([5, 7, 5, 7, 8, 8])}         # parts whose waves pad one factor at 5 and at 7


def waves_of(plan):
    """For each 64-lane wave of each round of plan["ent"]: the sorted parent counts of its valid lanes (bit 24 of word 1 is the valid
    flag, bits 16..23 hold the count).  A wave without a valid lane gives an empty list.  The kernels run a wave at the last one."""
    y = plan["ent"][:, 1].astype(np.int64)
    out = []
    for w in range(0, y.shape[0], 64):
        lane = y[w:w + 64]
        out.append(sorted(set(((lane[((lane >> 24) & 1) == 1] >> 16) & 0xff).tolist())))
    return out


def top_counts(plans):
    """the largest parent count of every non-empty wave of the plans (a plan, or the list of a several-workgroup plan's parts)"""
    plans = plans if isinstance(plans, list) else [plans]
    return [w[-1] for p in plans for w in waves_of(p) if w]


def padded_mixed_waves(plans):
    """the waves that run a padded instantiation at an odd count (5 or 7: every lane pads at least one factor) and also hold lanes
    with fewer parents"""
    plans = plans if isinstance(plans, list) else [plans]
    return [w for p in plans for w in waves_of(p) if w and w[-1] in (5, 7) and len(w) > 1]
