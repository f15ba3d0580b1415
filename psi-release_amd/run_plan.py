"""Planning of packed fitting runs over several scenes (pure Python: no torch, no GPU).

A run of the fused engine fits ``pack`` records at once; with ``independent_bodies`` the records of one run may live in different
scenes (``FittingOP.fitting_many(..., scene_ids=)``).  ``plan_runs`` turns per-scene work lists into such runs."""
from __future__ import annotations


def plan_runs(work_lists, pack):
    """``work_lists[s]``: the records (any objects) still to be fitted in scene slot ``s``; ``pack``: records per run.

    Returns ``(records, runs)``.  ``records`` is the flat work list, scene after scene in slot order, every record once.
    ``runs`` is a list of runs, each a list of exactly ``pack`` pairs ``(record index, slot)``: the records in flat order,
    ``pack`` at a time, so a run crosses from one scene into the next instead of leaving rows empty at every scene's end.
    Only the LAST run can be short of records; it is padded with copies of its last pair (the engine's batch size is fixed,
    the copies' results are dropped)."""
    pack = int(pack)
    if pack < 1:
        raise ValueError('pack must be at least 1')
    records, slots = [], []
    for s, lst in enumerate(work_lists):
        for rec in lst:
            records.append(rec)
            slots.append(s)
    runs = []
    for lo in range(0, len(records), pack):
        run = [(i, slots[i]) for i in range(lo, min(lo + pack, len(records)))]
        run += [run[-1]] * (pack - len(run))
        runs.append(run)
    return records, runs
