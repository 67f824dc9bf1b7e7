"""The schedule of a sketcher push (auriclass_amd/csrc/mhx_push_plan.h) as a plain statement, launch by launch.  Shared by
the push-plan tests; not a test module itself.

A sketcher has s, m, nslots, hash_max, admit_scale and two pairs of counters (bytes seen, next chunk), one for ordinary
pushes and one for repair passes.  A push is `n` bytes that begin `begin` (<= 15) bytes behind a 16-byte aligned base; its
tiles of TILE bytes are counted from that base.  Launch after launch takes some of the tiles that are left:

    the 64th launch of a push            all that is left
    m = 1                                next_chunk / TILE tiles (at least one); after every launch next_chunk grows by
                                         G = clamp(nslots / (16 s), GROWTH, 256) while it is below 2^40
    m > 1                                max(what is left of the first MiB, 7 x (3 x for m > 3) the bytes seen) / TILE tiles
    cap (m > 1)                          with `after` the bytes seen once this launch is done: none while after <= 1 MiB or
                                         f = 48 s' scale / after >= 1, s' = s + 8 sqrt(s) + 16; else max(1, floor(f hash_max))
    queue form                           the forced form if there is one; else never for format 0; else with the rate
                                         r = max(min(1, s / (0.4 bytes seen)) (1 when none), cap / hash_max):
                                         r <= 0.1 and (s >= 8192 or r > 3e-4)
    split                                1, except on the first launch of a push on a sketcher that has seen nothing, format
                                         not 1, no repair, no cap, inline form: the forced split, else the smallest power of
                                         two <= 8 with tiles x split >= cu_count (8 when none does)

The cap of a push's first launch is applied by a launch of its own (cap_before); the cap of every later launch rides with
the tighten pass of the launch before it (next_cap).  The pass behind the last launch checks the phase chain when the push
is format 2 or a repair pass and has two tiles or more.  Bytes seen advance by real bytes, not whole tiles.

Arithmetic in the 80-bit extended format of the host (numpy.longdouble), in the order the formulas are written.
"""
import numpy as np

LD = np.longdouble
TILE = 16384
MAX_LAUNCHES = 64
GROWTH = 16
UNCAPPED = 1 << 20
DEVICE_ORDER_MIN_SKETCH = 8192


def first_chunk(s, m, nslots):
    c0 = 1
    while c0 < 64 * s:
        c0 *= 2
    c0 = max(c0, 1 << 20)
    if m > 1:
        c0 = UNCAPPED
    return min(c0, nslots // 4)


def fresh_counters(s, m, nslots):
    c0 = first_chunk(s, m, nslots)
    return {"bytes": 0, "chunk": c0, "repair_bytes": 0, "repair_chunk": c0}


def tiles_of(begin, n):
    return (begin + n + TILE - 1) // TILE


def queue_form(kfmt, s, rate, forced=None):
    if forced is not None:
        return int(bool(forced))
    return int(kfmt != 0 and rate <= LD("0.1") and (s >= DEVICE_ORDER_MIN_SKETCH or rate > LD("3e-4")))


def cap_for(s, m, hash_max, scale, after):
    if m <= 1 or after <= UNCAPPED:
        return 0
    s_eff = LD(s) + LD(8) * np.sqrt(LD(s)) + LD(16)
    frac = LD(48) * s_eff * LD(scale) / LD(after)
    if not frac < LD(1):
        return 0
    return max(1, int(frac * LD(hash_max)))


def push(sk, counters, kfmt, repair, begin, n, cu_count, force_queue=None, force_split=0):
    """the launches of one push as dicts, in order; `counters` (fresh_counters) moves on"""
    s, m, nslots, hash_max, scale = sk
    kb, kc = ("repair_bytes", "repair_chunk") if repair else ("bytes", "chunk")
    ntiles = tiles_of(begin, n)
    before = counters[kb]
    growth = min(max(nslots // (16 * s), GROWTH), 256)
    out, tile = [], 0
    while tile < ntiles:
        seen = counters[kb]
        take = ntiles - tile
        if len(out) != MAX_LAUNCHES - 1:
            chunk = counters[kc] if m <= 1 else max(UNCAPPED - seen if seen < UNCAPPED else 0, (7 if m <= 3 else 3) * seen)
            take = min(take, max(1, chunk // TILE))
        after = before + min(n, (tile + take) * TILE)
        cap = cap_for(s, m, hash_max, scale, after)
        rate = min(LD(1), LD(s) / (LD("0.4") * LD(seen))) if seen else LD(1)
        if cap:
            rate = max(rate, LD(cap) / LD(hash_max))
        queue = queue_form(kfmt, s, rate, force_queue)
        split = 1
        if kfmt != 1 and not repair and before == 0 and not out and not cap and not queue:
            split = force_split or next((p for p in (1, 2, 4, 8) if take * p >= cu_count), 8)
        if out:
            out[-1]["next_cap"] = cap
        out.append({"tile0": tile, "ntiles": take, "split": split, "queue": queue, "cap_before": 0 if out else cap, "next_cap": 0, "verify": 0})
        tile += take
        counters[kb] = after
        if m <= 1 and counters[kc] < 1 << 40:
            counters[kc] *= growth
        out[-1]["bytes"], out[-1]["chunk"] = counters[kb], counters[kc]
    if out and (kfmt == 2 or repair) and ntiles >= 2:
        out[-1]["verify"] = 1
    return out
