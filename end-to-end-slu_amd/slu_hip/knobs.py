"""Readers of the SLU_* environment knobs with a closed set of values (no torch, no library: data.py imports this too).
The functions that own a knob keep its name, documentation and cross-knob rules; the parsing and the messages are here."""
import os


def flag(name, default="0"):
    """A 0/1 knob -> bool; any other value is a ValueError."""
    v = os.environ.get(name, default)
    if v not in ("0", "1"):
        raise ValueError("%s=%r: expected 0 or 1" % (name, v))
    return v == "1"


def one_of(name, default, allowed):
    """A knob that takes one of `allowed` -> that string; any other value is a ValueError naming them, sorted."""
    v = os.environ.get(name, default)
    if v not in allowed:
        raise ValueError("%s=%r: expected one of %s" % (name, v, sorted(allowed)))
    return v
