#!/usr/bin/env python
"""The exhaustive order check behind ranking through a link (DESIGN.md 4.2 "Ranking through a link").

c(x) = int32(phi(x) * 1e5) is what ranks compare under a non-linear score link.  libm's tanhf / expf / logf are not promised
monotone, so the per-row threshold bisection of emg_eval_link_thresholds is valid only under
    P(W): c(x_i) <= c(x_j) for all ordered non-NaN floats with j - i >= W.
This tool sweeps ALL floats (-inf .. +inf, both zeros) per link and W in {1, 2, 4, 8, 16, 32} with emg_eval_link_order_violations,
prints the violation counts and the time of each sweep, and names the smallest passing W per link — the value committed as
EMG_LINK_W_* in csrc/emg_common.hpp.  --locate also narrows a violation of the largest FAILING W down to a range of at most
65536 floats (bit patterns), by halving: the range tests/test_link_ranking.py keeps as its known violation.

    python tools/link_order_sweep.py [--locate]
"""
import argparse
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

from emgraph_amd import _lib as L  # noqa: E402
from emgraph_amd import device as D  # noqa: E402

K_MIN, K_MAX = 0x007FFFFF, 0xFF800000   # ordered keys of -inf and +inf
WS = (1, 2, 4, 8, 16, 32)


def key_to_bits(k):
    """ordered key -> IEEE bit pattern (the inverse of: sign flipped for x >= 0, all bits flipped for x < 0)"""
    return (k & 0x7FFFFFFF) if (k & 0x80000000) else (~k & 0xFFFFFFFF)


def sweep(link, W, k_lo=K_MIN, k_hi=K_MAX):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    n = int(D.eval_link_order_violations(link, W, key_to_bits(k_lo), key_to_bits(k_hi)).cpu()[0])
    return n, (time.perf_counter() - t0) * 1e3


def locate(link, W):
    """a range of <= 65536 keys holding a violation of P at this W (the halves overlap by the 2W floats a pair may span)"""
    lo, hi = K_MIN, K_MAX
    while hi - lo > 65536:
        mid = lo + (hi - lo) // 2
        if sweep(link, W, lo, mid)[0] > 0:
            hi = mid
        elif sweep(link, W, mid - 2 * W, hi)[0] > 0:
            lo = mid - 2 * W
        else:
            raise AssertionError("violation lost while halving")
    return lo, hi


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--locate", action="store_true", help="narrow a violation of the largest failing W down to <= 65536 floats")
    args = ap.parse_args()
    D.require_gpu()
    print("torch %s  hip %s  device %s" % (torch.__version__, torch.version.hip, torch.cuda.get_device_name(0)))
    sweep(L.LINK_TANH, 1, K_MAX - 4096, K_MAX)   # (first launch: module load)
    for name in ("tanh", "sigmoid", "softplus"):
        link = L.LINK_IDS[name]
        smallest, failing = None, None
        for W in WS:
            n, ms = sweep(link, W)
            print("%-8s W=%-2d violations=%-12d sweep_ms=%.1f" % (name, W, n, ms), flush=True)
            if n == 0 and smallest is None:
                smallest = W
            if n > 0:
                failing = W
        print("%-8s smallest passing W: %s   committed: %d" % (name, smallest, D.link_order_w(link)), flush=True)
        if args.locate and failing is not None:
            lo, hi = locate(link, failing)
            print("%-8s violation of W=%d inside bits [0x%08x, 0x%08x] (%d there)"
                  % (name, failing, key_to_bits(lo), key_to_bits(hi), sweep(link, failing, lo, hi)[0]), flush=True)
    n, ms = sweep(L.LINK_TANH | 0x100, 1)
    print("planted (negated tanh) W=1 violations=%d sweep_ms=%.1f" % (n, ms))


if __name__ == "__main__":
    main()
