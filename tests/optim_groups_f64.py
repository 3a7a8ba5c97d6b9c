"""TEST INFRASTRUCTURE: the float64 reference of a grouped optimizer-side step (calm_optim_step_groups), built from
tail_f64.optim_reference without new arithmetic and without a new tolerance.  The norm, the clip coefficient, found_inf
and the step count do not depend on lr / weight_decay, so evaluating the ungrouped reference over the WHOLE table once
per group, with that group's (lr, weight_decay), gives the same global quantities every time; the elements of a group's
tensors are then taken from that group's result and from its bounds."""
import torch

import tail_f64 as tf

# three groups that differ in both values, one of them with lr = 0 (parameters frozen, moments moving), and a fourth
# group that no tensor is in
GROUP_HP = [(1e-3, 0.05), (2.5e-4, 0.0), (0.0, 0.05), (7e-4, 0.01)]
SCENARIOS = ("no_clip_t1", "clip_t1000", "below_t2", "scaled_t100000")
WRONG_LR, WRONG_WD = 0.5, 0.9                 # hp.lr / hp.weight_decay of a grouped call: ignored by the entry point


def scenario(name):
    return next(s for s in tf.OPTIM_SCENARIOS if s["name"] == name)


def table_groups(table):
    """Tensor k in group k % 3, except that the multi-chunk tensor (3 C + 5 elements), the two spectral-norm tensors of more
    than one chunk, whose chunk boundary falls inside a row, and the cancelling tensor sit in groups 1 and 2."""
    groups = [k % 3 for k in range(len(table))]
    pinned = {("plain", 3 * tf.OPT_CHUNK + 5): 1, ("sn", 144 * 288): 1, ("sn", 300 * 260): 2, ("cancel", 64 * 48): 2}
    seen = set()
    for k, e in enumerate(table):
        key = (e["kind"], e["numel"])
        if key in pinned:
            groups[k] = pinned[key]
            seen.add(key)
    assert seen == set(pinned)
    return groups


def hp_of(sc, lr=WRONG_LR, wd=WRONG_WD):
    """(lr, beta1, beta2, eps, weight_decay, max_norm, step) of a scenario with the given rate and decay"""
    return (lr, tf.OPT_BETA1, tf.OPT_BETA2, tf.OPT_EPS, wd, sc["max_norm"], 0)


def element_groups(recs, groups):
    """the group of every element of the flat concatenation"""
    return torch.cat([torch.full((r["param"].numel(),), g, dtype=torch.int64) for r, g in zip(recs, groups)])


def grouped_reference(recs, grads, sc, group_hp, groups, step):
    """-> (ref, bound) in the form of tail_f64.optim_reference, p / m / v and their bounds assembled per group."""
    owner = element_groups(recs, groups)
    ref = bound = None
    for g, (lr, wd) in enumerate(group_hp):
        mine = owner == g
        if not bool(mine.any()):
            continue
        r, b = tf.optim_reference(recs, grads, hp_of(sc, lr, wd), sc["grad_scale"], step)
        if ref is None:
            ref, bound = dict(r), dict(b)
            for k in ("p", "m", "v"):
                ref[k] = r[k].clone()
                if k in b:
                    bound[k] = b[k].clone()
            continue
        # what does not depend on the rates is equal, to the last bit, in every evaluation
        assert (r["found_inf"], r["step"]) == (ref["found_inf"], ref["step"])
        assert r["found_inf"] == 1.0 or (r["norm"], r["clip"], b["norm"]) == (ref["norm"], ref["clip"], bound["norm"])
        for k in ("p", "m", "v"):
            ref[k][mine] = r[k][mine]
            if k in b:
                bound[k][mine] = b[k][mine]
    return ref, bound


def with_groups(recs, groups):
    """the records with their "group" key (what OptimPlan and the torch fallback read)"""
    return [dict(r, group=g) for r, g in zip(recs, groups)]
