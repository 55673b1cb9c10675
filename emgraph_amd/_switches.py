"""The environment variables the Python package reads: one declared table, one reader.  Every variable is read at the call
that uses it (a Trainer decides at construction, an evaluation per call), so a test may set one between two calls of one
process.  The library's own table is emgraph_amd/csrc/emg_abi.hip; DESIGN.md "Environment switches" lists both, with the
test that compares each switch's forms (tests/test_switches.py holds the three to the same names)."""
from __future__ import annotations

import os

# name -> (default, doc); default None = unset
SWITCHES = {
    "EMG_ADAM_DEFERRED": (None, "0 | 1: the deferred dense pass off / forced; unset: entity tables of 256 MB or more"),
    "EMG_FACTORED": ("1", "0: full gradient rows instead of factored contributions"),
    "EMG_GROUPING": (None, "also read by the library (the grouping backend); here: sort = the host-driven exchange of batch sharding"),
    "EMG_INPLACE_STATE": ("1", "0: a stateful optimizer's in-place updates without the window form"),
    "EMG_INPLACE": (None, "0 | 1: in-place singleton updates off / forced where they can run"),
    "EMG_GRAPH": (None, "0 | 1: steps as graph replays off / forced where the plan can; unset: small batches"),
    "EMG_RESCORE": ("segments", "segments | tiles: the exact re-scoring form"),
    "EMG_PREFILTER_PROBE": ("1", "0: precision 2 (and RotatE's exact-fast mode) without the probe"),
    "EMG_PREFILTER_TIES": ("1", "0: precision 2 without the ties-proving form"),
    # configuration, not A/B
    "EMG_PAIR_CAP": ("2048", "configuration: pair-buffer entries per wave"),
    "EMG_PAIR_LOG2": ("29", "configuration: log2 of the pair buffer's entries in total"),
    "EMG_SHARDING": ("k", "configuration: k | batch, the multi-GPU plan"),
    "EMG_EVAL_PRECISION": ("auto", "configuration: 0 | 1 | 2 | auto, the ranking path"),
    "EMGRAPH_HIP_LIB": (None, "configuration: path of a variant libemgraph_hip.so"),
}


def get(name):
    """the variable's value, or its declared default; an undeclared name is an error"""
    return os.environ.get(name, SWITCHES[name][0])
