#!/usr/bin/env python
"""Host cost of a C-ABI call through the host mirrors, one source tree against another (the kernels being the same, what differs
is how the Python side reaches them: device guard, stream lookup, pointer conversion, status check).

    python tools/host_call_probe.py --parent DIR --branch DIR [--ids PARENT BRANCH] [--rounds 2] [--bench [--dump DIR]]
                                    [--out profiles/host_call_probe.txt]
    python tools/host_call_probe.py --tree DIR          (what the first form starts: one JSON line of us per call)

Launch-bound calls at toy sizes, so that the call overhead is what is timed:
    ema       ema_update_flat_ on 4096 elements
    lsap      lsap_batch on one 16 x 4 problem
    select    select_queries at N=1, S=1024, C=8, k=64, d_model=32
    addnorm   add_layer_norm forward + backward on (2, 300, 256)
    attn      masked_attention forward + backward at Lq = Lk = 64, B = 1, 8 heads
    consis    consistency_loss forward + backward at L = 2, B = 1, Q = 32, K = 8, D = 256
Wall time per call over at least 100 calls and at least 0.25 s after 20 warm-up calls, including the final synchronize.  Every
measurement is a fresh child process that imports the package from its tree (each tree needs its built library); the trees
alternate, ``--rounds`` times each, and the table gives min .. max per tree.  The branch passes where its minimum is no higher
than the parent's maximum: the parent's own spread is the margin on a shared host.  ``--bench`` adds the headline of
``bench.py --gpus 1 --steps 10 --warmup 3`` of both trees the same way (images/s: branch's best no lower than parent's worst);
``--dump DIR`` has every one of these bench runs write its ``--dump-outputs`` to ``DIR/parent<i>`` / ``DIR/branch<i>``, for the
output-by-output comparison of the two trees.  The exit status is 1 when a row says SLOWER.
"""
import argparse
import json
import os
import subprocess
import sys
import time

CALLS = ("ema", "lsap", "select", "addnorm", "attn", "consis")


def wall(fn, sync, calls=100, warmup=20, min_seconds=0.25):
    for _ in range(warmup):
        fn()
    sync()
    t0 = time.perf_counter()
    for _ in range(10):
        fn()
    sync()
    calls = max(calls, int(min_seconds / max((time.perf_counter() - t0) / 10, 1e-6)))
    t0 = time.perf_counter()
    for _ in range(calls):
        fn()
    sync()
    return (time.perf_counter() - t0) / calls * 1e6


def measure(tree):
    sys.path.insert(0, os.path.abspath(tree))
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("host_call_probe: needs a GPU (no timing is taken on the CPU)")
    import semi_detr_amd as s
    from semi_detr_amd.matcher import lsap_batch
    assert os.path.abspath(s.__file__).startswith(os.path.abspath(tree) + os.sep), s.__file__
    dev = torch.device("cuda:0")
    g = torch.Generator(device=dev).manual_seed(0)
    teacher, student = torch.randn(4096, device=dev, generator=g), torch.randn(4096, device=dev, generator=g)
    Q, G = 16, 4
    cost = torch.rand(G * Q, device=dev, generator=g)
    offs = [0, G]
    offs_dev = torch.tensor(offs, dtype=torch.int32, device=dev)
    N, S, C, k, D = 1, 1024, 8, 64, 32
    logits = torch.randn(N, S, C, device=dev, generator=g)
    coord, prop = torch.randn(N, S, 4, device=dev, generator=g), torch.randn(N, S, 4, device=dev, generator=g)
    memory = torch.randn(N, S, D, device=dev, generator=g)

    def leaves(*shape, n=1):
        return [torch.randn(*shape, device=dev, generator=g).requires_grad_(True) for _ in range(n)]

    def train(forward, inputs, grads):           # forward + backward without accumulating into .grad
        def run():
            with torch.enable_grad():
                torch.autograd.grad(forward(), inputs, grads)
        return run
    xr, wb, qkv = leaves(2, 300, 256, n=2), leaves(256, n=2), leaves(64, 1, 256, n=3)
    hs1, hs2 = leaves(1, 32, 256, n=2), [t.detach() for t in leaves(1, 32, 256, n=2)]
    meta = {"pad_size_1": 8, "known_bid_1": torch.zeros(8, device=dev), "map_known_indice_1": torch.arange(8, device=dev),
            "loss_weights": torch.ones(8, 1, device=dev)}
    one = torch.ones((), device=dev)
    fns = {"ema": lambda: s.ema_update_flat_(teacher, student, 0.999),
           "lsap": lambda: lsap_batch(cost, offs_dev, offs, Q),
           "select": lambda: s.select_queries(logits, coord, prop, memory, k),
           "addnorm": train(lambda: s.add_layer_norm(*xr, *wb), xr + wb, torch.ones(2, 300, 256, device=dev)),
           "attn": train(lambda: s.masked_attention(*qkv, 8), qkv, torch.ones(64, 1, 256, device=dev)),
           "consis": train(lambda: list(s.consistency_loss(hs1, hs2, meta).values()), hs1, [one, one])}
    with torch.no_grad():
        res = {name: wall(fns[name], torch.cuda.synchronize) for name in CALLS}
    res["device"] = torch.cuda.get_device_name(0)
    print(json.dumps(res))


def child(argv, timeout):
    """A fresh process; its last stdout line is the JSON result.  A failure ends the whole probe: nothing more is started."""
    r = subprocess.run(argv, stdout=subprocess.PIPE, text=True, timeout=timeout)
    if r.returncode != 0:
        raise SystemExit(f"host_call_probe: {' '.join(argv)} exited with {r.returncode}")
    return json.loads(r.stdout.strip().splitlines()[-1])


def span(v):
    return f"{min(v):9.2f} .. {max(v):9.2f}"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tree")
    ap.add_argument("--parent")
    ap.add_argument("--branch")
    ap.add_argument("--ids", nargs=2, default=["?", "?"], metavar=("PARENT", "BRANCH"), help="commit ids for the report")
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--bench", action="store_true")
    ap.add_argument("--dump", metavar="DIR", help="with --bench: pass --dump-outputs DIR/<tree><round> to every bench run")
    ap.add_argument("--out")
    a = ap.parse_args()
    if a.tree:
        measure(a.tree)
        return 0
    if not (a.parent and a.branch):
        ap.error("give --tree DIR, or --parent DIR and --branch DIR")
    trees = {"parent": os.path.abspath(a.parent), "branch": os.path.abspath(a.branch)}
    runs = {t: [] for t in trees}
    missed = 0
    for _ in range(a.rounds):
        for t, path in trees.items():
            runs[t].append(child([sys.executable, os.path.abspath(__file__), "--tree", path], 300))
    lines = [f"{runs['parent'][0]['device']}; parent {a.ids[0]}, branch {a.ids[1]}; wall time per call in us over at least 100 "
             f"calls and at least 0.25 s after 20 warm-up calls, incl. the final synchronize; fresh child processes, {a.rounds} "
             f"alternating rounds per tree, min .. max"]
    for name in CALLS:
        p, b = [r[name] for r in runs["parent"]], [r[name] for r in runs["branch"]]
        verdict = "no slower" if min(b) <= max(p) else "SLOWER"
        missed += verdict == "SLOWER"
        lines.append(f"{name:7s} parent {span(p)}   branch {span(b)}   branch min / parent min {min(b) / min(p):5.2f}   "
                     f"{verdict}")
    if a.bench:
        bench = {t: [] for t in trees}
        for i in range(a.rounds):
            for t, path in trees.items():
                argv = [sys.executable, os.path.join(path, "bench.py"), "--gpus", "1", "--steps", "10", "--warmup", "3"]
                if a.dump:
                    argv += ["--dump-outputs", os.path.join(a.dump, f"{t}{i}")]
                bench[t].append(child(argv, 900))
        p, b = [r["value"] for r in bench["parent"]], [r["value"] for r in bench["branch"]]
        r0 = bench["parent"][0]
        lines.append(f"bench.py --gpus 1 --steps 10 --warmup 3, {r0['metric']} in {r0['unit']}, {a.rounds} alternating runs per "
                     f"tree")
        missed += max(b) < min(p)
        lines.append(f"bench   parent {span(p)}   branch {span(b)}   branch best / parent best {max(b) / max(p):5.3f}   "
                     f"{'no slower' if max(b) >= min(p) else 'SLOWER'}")
    text = "\n".join(lines)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        open(a.out, "w").write(text + "\n")
    return 1 if missed else 0


if __name__ == "__main__":
    sys.exit(main())
