"""Precision schedules: which engine precision takes which step of one sampling run.

A schedule is ``NAME[:COUNT](,NAME[:COUNT])*`` - ``"bf16:40,f16x3"`` is "the first 40 loop indices in bf16, the rest in f16x3",
``"bf16,f16x3:10"`` "the last 10 in f16x3" - or the same thing as a sequence of ``(name, count or None)`` pairs.  The sampler's
canvases are fp32 in every precision and the noise draws do not depend on the engine, so a run may change engines between two
steps without a conversion.  Pure Python: importable without torch or a GPU.
"""
import re
from typing import List, Optional, Sequence, Tuple, Union

# the keys of srgd_amd.engine._PRECISIONS, restated so that this module needs no torch (tests/test_precision_schedule_cpu.py
# holds the two together)
PRECISION_NAMES = ("fp32", "bf16", "bf16_w8", "fp8", "fp8_mixed", "f16x3", "f16mx2", "f16x1")
MAX_ENTRIES = 4

Schedule = Tuple[Tuple[str, Optional[int]], ...]
_INTEGER = re.compile(r"[+-]?[0-9]+\Z")


def _entry_of_token(token: str):
    text = token.strip()
    if not text:
        raise ValueError(f"precision schedule: empty entry {token!r} (entries are NAME or NAME:COUNT)")
    name, sep, count = text.partition(":")
    name, count = name.strip(), count.strip()
    if not name:
        raise ValueError(f"precision schedule: entry {text!r} has no precision name")
    if not sep:
        return name, None, text
    if not _INTEGER.match(count):
        raise ValueError(f"precision schedule: the count of {text!r} is not an integer")
    return name, int(count), text


def _entry_of_pair(pair):
    try:
        name, count = pair
    except (TypeError, ValueError):
        raise ValueError(f"precision schedule: entry {pair!r} is not a (name, count or None) pair") from None
    if not isinstance(name, str) or not name.strip():
        raise ValueError(f"precision schedule: empty entry {pair!r} (the name of a pair is a precision name)")
    if count is not None and (isinstance(count, bool) or not isinstance(count, int)):
        raise ValueError(f"precision schedule: the count of {pair!r} is not an integer")
    return name.strip(), count, repr(pair)


def parse_schedule(spec: Union[str, Sequence]) -> Schedule:
    """The entries ``((name, count or None), ...)`` of a schedule given as a string or as a sequence of pairs: 1 to 4 entries, every
    name a precision of the engine, every count an integer >= 1, at most one entry without a count (it takes the rest of the run).
    Anything else is a ``ValueError`` that names the offending token."""
    if isinstance(spec, str):
        entries = [_entry_of_token(t) for t in spec.split(",")]
    elif isinstance(spec, (list, tuple)):
        if not spec:
            raise ValueError("precision schedule: empty entry (a schedule has 1 to 4 entries)")
        entries = [_entry_of_pair(p) for p in spec]
    else:
        raise ValueError(f"precision schedule: {spec!r} is neither a string nor a sequence of (name, count or None) pairs")
    if len(entries) > MAX_ENTRIES:
        raise ValueError(f"precision schedule: more than {MAX_ENTRIES} entries, the first too many is {entries[MAX_ENTRIES][2]}")
    rest = None
    for name, count, shown in entries:
        if name not in PRECISION_NAMES:
            raise ValueError(f"precision schedule: unknown precision {name!r} in {shown} (one of {', '.join(PRECISION_NAMES)})")
        if count is None:
            if rest is not None:
                raise ValueError(f"precision schedule: more than one entry without a count ({rest} and {shown}); only one takes the rest")
            rest = shown
        elif count < 1:
            raise ValueError(f"precision schedule: the count of {shown} must be >= 1")
    return tuple((name, count) for name, count, _ in entries)


def plan_steps(schedule: Union[str, Sequence], num_sample_steps: int) -> List[str]:
    """One precision name per loop index ``0 .. num_sample_steps - 1`` of the sampling loop (absolute indices: those below
    ``generation_start_steps`` are planned like the others and not run).  The entry without a count takes what the counted ones
    leave, which may be nothing.  ``ValueError``: counts above ``num_sample_steps``, or a fully counted schedule of another sum."""
    entries = parse_schedule(schedule)
    if isinstance(num_sample_steps, bool) or not isinstance(num_sample_steps, int) or num_sample_steps < 1:
        raise ValueError(f"precision schedule: num_sample_steps must be an integer >= 1, got {num_sample_steps!r}")
    counted = sum(c for _, c in entries if c is not None)
    shown = format_runs([(n, c) for n, c in entries])
    if counted > num_sample_steps:
        raise ValueError(f"precision schedule: the counts of {shown!r} sum to {counted}, above the run's {num_sample_steps} steps")
    if all(c is not None for _, c in entries) and counted != num_sample_steps:
        raise ValueError(f"precision schedule: the counts of {shown!r} sum to {counted}, the run has {num_sample_steps} steps "
                         "(leave one count out: that entry takes the rest)")
    plan: List[str] = []
    for name, count in entries:
        plan += [name] * (num_sample_steps - counted if count is None else count)
    return plan


def plan_runs(plan: Sequence[str]) -> List[Tuple[str, int]]:
    """``[(name, steps)]`` of a plan with adjacent steps of one name merged."""
    runs: List[Tuple[str, int]] = []
    for name in plan:
        if runs and runs[-1][0] == name:
            runs[-1] = (name, runs[-1][1] + 1)
        else:
            runs.append((name, 1))
    return runs


def format_runs(runs: Sequence[Tuple[str, Optional[int]]]) -> str:
    """A schedule or the runs of a plan in the string spelling, ``bf16:40,f16x3:10``."""
    return ",".join(name if count is None else f"{name}:{count}" for name, count in runs)


def describe_plan(plan: Sequence[str]) -> str:
    """The runs of a plan as the command line prints them, ``bf16 x40, f16x3 x10``."""
    return ", ".join(f"{name} x{count}" for name, count in plan_runs(plan))


def executed_names(plan: Sequence[str], generation_start_steps: int = 0) -> List[str]:
    """The distinct names of the steps a run executes, in order of first use (a run that executes none: the plan's last name, whose
    engine makes the start and end calls)."""
    names: List[str] = []
    for name in plan[max(0, int(generation_start_steps)):]:
        if name not in names:
            names.append(name)
    return names or [plan[-1]]
