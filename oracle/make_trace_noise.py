#!/usr/bin/env python3
"""How fast fp32 trajectories of the G22 recipes part, measured on the CPU port -> tests/golden/G23_trace_noise.npz.

tests/test_hip_train_trace.py allows the HIP trainer 8 x the distance between control runs of the HIP trainer itself; this file
measures the same quantity with arithmetic that is not under test, so that the HIP controls' own distance gets a ceiling
(tests/_trace_noise.py has the derivation).  Per trace (kplanes, vanilla, kplanes_lr): one unperturbed replay of
``oracle/torch_port.reference_training`` with the arguments of tests/test_oracle_train_trace._replay, and six control replays whose
floating parameters (all but ``*freqs``) are multiplied by 1 + 2^-22 (U - 0.5), U uniform per element from
``torch.Generator().manual_seed(control)`` -- the rule of test_hip_train_trace._run(perturb=...), on the CPU.

CPU only; reads the port and tests/golden/G22_*, nothing of the reference.  The replays are independent: ``--jobs J`` runs J at a
time, each a fresh child process with (CPUs available to this process) // J torch threads.  ~45 CPU-minutes serial (the 70-step trace
is ~6 min per replay).

    python oracle/make_trace_noise.py --jobs 8 [--out tests/golden/G23_trace_noise.npz]
"""
import argparse
import os
import subprocess
import sys
import tempfile
import time

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

import _g22                                  # noqa: E402
import _trace_noise as tn                    # noqa: E402
from oracle import torch_port as tp          # noqa: E402

CONTROLS = (1, 2, 3, 4, 5, 6)
AMPLITUDE = 2.0 ** -22


def perturbed_state(method, seed, control):
    """the port's initial state; for control > 0 every floating parameter except ``*freqs`` times 1 + AMPLITUDE (U - 0.5)"""
    sd = tp.initial_state(method, seed)
    if control:
        gen = torch.Generator().manual_seed(control)
        for k, v in sd.items():
            if v.is_floating_point() and not k.endswith("freqs"):
                sd[k] = v * (1.0 + AMPLITUDE * (torch.rand(v.shape, generator=gen) - 0.5))
    return sd


def replay(name, control, n_steps=None):
    """-> (per-step losses [K] float64, name -> what ``_g22.compare_final_state`` compares of the final state)"""
    g = _g22.trace(name)
    o, d, rgbs, bg = _g22.ray_table()
    method, seed, K = str(g["method"]), int(g["seed"]), int(g["steps"]) if n_steps is None else n_steps
    losses, sd, _ = tp.reference_training(perturbed_state(method, seed, control), o, d, rgbs, method=method, batch_size=int(g["batch_size"]),
                                          n_samples=int(g["n_samples"]), n_steps=K, bg=tuple(bg.tolist()), replay={"seed": seed, "rank": 0},
                                          loader="dataloader")
    seen = {}
    for n in g["param_names"]:
        n = str(n)
        a = np.ascontiguousarray(sd[n].numpy())
        seen[n] = a if "final/" + n in g else a.ravel()[_g22.subsample_index(a.size)]
    return np.array(losses, np.float64), seen


def spread_of(control, unperturbed, names):
    """[N]: max |control - unperturbed| / max |unperturbed| per recorded parameter"""
    return np.array([float(np.abs(control[n].astype(np.float64) - unperturbed[n]).max() / max(float(np.abs(unperturbed[n]).max()), 1e-30))
                     for n in names])


def available_cpus():
    return len(os.sched_getaffinity(0)) if hasattr(os, "sched_getaffinity") else 1


def child(name, control, threads, path):
    torch.set_num_threads(threads)
    losses, seen = replay(name, control)
    np.savez(path, loss=losses, **{"p/" + n: a for n, a in seen.items()})


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "G23_trace_noise.npz"))
    ap.add_argument("--jobs", type=int, default=1)
    ap.add_argument("--traces", nargs="+", default=list(tn.TRACES))
    ap.add_argument("--work", help="keep every replay's result in this directory and reuse what is already there")
    ap.add_argument("--child", nargs=4, metavar=("TRACE", "CONTROL", "THREADS", "FILE"), help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.child:
        return child(a.child[0], int(a.child[1]), int(a.child[2]), a.child[3])
    jobs = max(1, a.jobs)
    threads = max(1, available_cpus() // jobs)
    steps = {t: int(_g22.trace(t)["steps"]) for t in a.traces}
    todo = sorted(((t, c) for t in a.traces for c in (0,) + CONTROLS), key=lambda tc: -steps[tc[0]])          # the long replays first
    out = {"controls": np.array(CONTROLS), "amplitude": np.float64(AMPLITUDE), "threads": np.int64(threads), "traces": np.array(a.traces)}
    with tempfile.TemporaryDirectory() as tmp:
        work = a.work or tmp
        os.makedirs(work, exist_ok=True)
        path = lambda t, c: os.path.join(work, f"{t}_{c}.npz")
        todo = [tc for tc in todo if not os.path.exists(path(*tc))]          # (--work: replays already there are kept)
        running, failed = [], []
        while todo or running:
            while todo and len(running) < jobs:
                t, c = todo.pop(0)
                running.append((t, c, subprocess.Popen([sys.executable, os.path.abspath(__file__), "--child", t, str(c), str(threads), path(t, c)])))
            time.sleep(0.5)
            for r in [r for r in running if r[2].poll() is not None]:
                running.remove(r)
                print(f"{r[0]} control {r[1]}: exit {r[2].returncode}", flush=True)
                if r[2].returncode != 0:
                    failed.append(r[:2])
        if failed:
            raise SystemExit(f"replays failed: {failed}")
        for t in a.traces:
            g = _g22.trace(t)
            names = [str(n) for n in g["param_names"]]
            runs = {c: np.load(path(t, c)) for c in (0,) + CONTROLS}
            base = {n: runs[0]["p/" + n] for n in names}
            loss = np.stack([runs[c]["loss"] for c in CONTROLS])
            spread = np.stack([spread_of({n: runs[c]["p/" + n] for n in names}, base, names) for c in CONTROLS])
            out.update({f"{t}/loss": loss, f"{t}/spread": spread, f"{t}/unperturbed_loss": runs[0]["loss"], f"{t}/param_names": np.array(names)})
            d = tn.derive(loss, spread, g["loss"])
            out.update({f"{t}/{k}": v for k, v in d.items()})
            print(t, "R", float(d["R"]), "R_p", float(d["R_p"]), "E6[-1]", d["E6"][-1], "S6 max", d["S6"].max(),
                  "unperturbed / record - 1:", float(np.abs(runs[0]["loss"] / g["loss"] - 1).max()))
    np.savez_compressed(a.out, **out)
    print("wrote", a.out, os.path.getsize(a.out), "bytes")


if __name__ == "__main__":
    main()
