#!/usr/bin/env python3
"""LDS bank-conflict table of the Stockham passes of csrc/fft_lds.h (no GPU needed: it counts addresses).

    python tools/fft_lds_conflicts.py

Model (MI355X LDS, 8-byte elements): a 64-lane ``ds_read_b64`` is served in two groups of 32 lanes over 32 eight-byte slots
(64 banks of 4 bytes), a ``ds_write_b64`` in four groups of 16 contiguous lanes over 16 slots (32 banks); within a group,
every further DISTINCT address on a busy slot costs one more LDS cycle, equal addresses broadcast.  Per pass (radix R, Ns
done) of a plan, for the three access streams -- data read buf[j + r N / R], twiddle read tw[r k N / (R Ns)], scatter write
buf[(j - k) R + k + r Ns] -- it prints the worst number of distinct addresses on one slot, and per plan the sum over all
accesses of the mean per-group degree (a relative cost, not a time).  The comment above ``fpad`` in fft_lds.h quotes it.
"""

PADS = {"none": lambda i: i, "i + (i >> 5)": lambda i: i + (i >> 5), "i + (i >> 4)": lambda i: i + (i >> 4)}
PLANS = {1200: [[8, 6, 5, 5], [5, 5, 6, 8], [5, 5, 8, 6], [6, 8, 5, 5], [5, 8, 6, 5], [5, 6, 8, 5], [4, 4, 3, 5, 5]],
         400: [[8, 2, 5, 5], [5, 5, 4, 4], [4, 4, 5, 5]], 240: [[8, 6, 5], [5, 6, 8], [5, 3, 4, 4]], 2048: [[8, 8, 8, 4]]}


def degree(addrs, group, slots):
    worst, total, n = 1, 0, 0
    for g0 in range(0, len(addrs), group):
        g = {a for a in addrs[g0:g0 + group] if a is not None}
        if not g:
            continue
        per_slot = {}
        for a in g:
            per_slot[a % slots] = per_slot.get(a % slots, 0) + 1
        d = max(per_slot.values())
        worst, total, n = max(worst, d), total + d, n + 1
    return worst, total / max(n, 1)


def analyse(N, plan, pad):
    NS, rows, total = 1, [], 0.0
    for R in plan:
        NB, TS = N // R, N // (R * NS)
        rd = tw = wr = 1
        for i in range((NB + 255) // 256):
            js = [t + 256 * i if t + 256 * i < NB else None for t in range(256)]
            for r in range(R):
                w, c = degree([None if j is None else pad(j + r * NB) for j in js], 32, 32)
                rd, total = max(rd, w), total + c
                if NS > 1 and r > 0:
                    w, c = degree([None if j is None else pad(r * (j % NS) * TS) for j in js], 32, 32)
                    tw, total = max(tw, w), total + c
                w, c = degree([None if j is None else pad((j - j % NS) * R + j % NS + r * NS) for j in js], 16, 16)
                wr, total = max(wr, w), total + c
        rows.append(f"({R}, {NS}) {rd} / {tw if NS > 1 else '-'} / {wr}")
        NS *= R
    return rows, total


def main():
    print("per pass: (radix, Ns) worst data read / twiddle read / write")
    for N, plans in PLANS.items():
        for plan in plans:
            for name, pad in PADS.items():
                rows, total = analyse(N, plan, pad)
                print(f"{N:5d} = {' * '.join(map(str, plan)):<18} pad {name:<13} cost {total:6.1f}   " + "   ".join(rows))


if __name__ == "__main__":
    main()
