"""Numpy twin of the per-tile adaptive loop (include/mirt.h, "per-tile adaptive sampling"), built on noise_twin.py.

The freeze rule, for a tile that is not yet frozen, from its record {max, mean, usable, nonfinite} and `above` = its usable pixels with
e > target:  freeze  <=>  nonfinite == 0  and  above <= (uint32)floor((1.0 - quantile) * usable), the arithmetic in double.

The loop: accumulate check_every, estimate, select, freeze — nothing freezes before min_accumulations — until every tile is frozen or
max_accumulations is reached.  A frozen tile holds what `count` plain accumulations leave in it, so the loop can be replayed from the plain
accumulator at every check: replay() takes a function n -> slab [tiles][k][3][256] after n plain accumulations."""
import math

import numpy as np

import noise_twin as nt

f32 = np.float32

# The end-to-end scene of the tests: default9 at 64 x 64, buckets 5, max_bounces 5, check_every 5.  TARGET was picked on the CPU (oracle +
# this twin) so that the loop freezes tiles at its first check and still has active tiles at its last; test_adaptive_cpu.py asserts both.
SCENE = {"width": 64, "height": 64, "buckets": 5, "max_bounces": 5, "check_every": 5, "quantile": 0.95, "floor": 0.0, "max_accumulations": 30}
TARGET = 0.6
TARGET_ALL_FREEZE = 1e30          # every tile freezes at the first check: the MIRT_OK branch


def select(records, above, frozen, quantile):
    records = np.asarray(records, dtype=f32).reshape(-1, 4)
    out = np.zeros(len(records), dtype=np.uint8)
    for t, (rec, a) in enumerate(zip(records, above)):
        if frozen is not None and frozen[t]:
            out[t] = 1
            continue
        cut = int(math.floor((1.0 - float(quantile)) * float(rec[2])))
        out[t] = 1 if (rec[3] == 0 and int(a) <= cut) else 0
    return out


def above_of(e, target):
    """e [tiles][256] -> usable pixels per tile with e > target."""
    e = np.asarray(e, dtype=f32)
    with np.errstate(invalid="ignore"):
        return (nt.usable(e) & (e > f32(target))).sum(axis=1).astype(np.uint32)


def records_of(e):
    t_max, t_mean, n_ok, n_bad = nt.tile_records(e)
    return np.stack([t_max, t_mean.astype(f32), n_ok.astype(f32), n_bad.astype(f32)], axis=1)


def replay(slab_at, n_tiles, exposure, target, quantile, floor, k, check_every, min_accumulations, max_accumulations, start=0, select_fn=None):
    """-> {"converged", "issued", "checks", "counts" [tiles], "masks": [frozen mask after each check]}.  select_fn: another implementation of
    select(), asked beside it at every check; its answer must be the same."""
    frozen = np.zeros(n_tiles, dtype=np.uint8)
    counts = np.zeros(n_tiles, dtype=np.uint32)
    acc, checks, masks = start, 0, []
    while True:
        if frozen.all():
            converged = True
            break
        room = max(max_accumulations - acc, 0)
        step = room - room % k if room < check_every else check_every
        if step == 0:
            converged = False
            break
        acc += step
        checks += 1
        e = nt.noise_e(slab_at(acc), nt.scale_of(exposure, acc, k), floor)
        if acc >= min_accumulations:
            new = select(records_of(e), above_of(e, target), frozen, quantile)
            if select_fn is not None:
                assert np.array_equal(np.asarray(select_fn(records_of(e), above_of(e, target), frozen, quantile)), new), f"select at {acc} accumulations"
            counts[(new != 0) & (frozen == 0)] = acc
            frozen = new
        masks.append(frozen.copy())
    counts[frozen == 0] = acc
    return {"converged": converged, "issued": acc - start, "checks": checks, "counts": counts, "masks": masks}
