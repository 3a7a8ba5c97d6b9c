#!/usr/bin/env python3
"""A/B record of trainer.train() (not a test): runs train() over a matrix of configurations on the test suite's tiny
models (tiny32_cls, nano48_gen for task="reg"; batch 4, two epochs, 10 - 14 samples so the last batch and the last
accumulation window are partial, log_every=1) and writes one JSON line per run:

    {"name", "stdout": captured lines, "state_sha256": sha256 of the returned state_dict's bytes in key order,
     "files": sorted [[relative path, sha256], ...] of everything the run wrote}

Run it on two trees (two commits) and compare the outputs: a refactor of train() must leave them equal line for line.

    train_ab.py --device cpu|gpu --out FILE [--tree DIR] [--only NAME[,NAME]]
    train_ab.py --compare A.jsonl B.jsonl [--masked NAME[,NAME]]

--tree: the checkout whose package and test helpers are imported (default: this one).  Every configuration runs in a
fresh child process under its own time limit, one at a time; the first failing child stops the script.  --masked: the
named runs are compared on stdout with the numbers masked and on the set of files written (for runs that differ between
two runs of the same code)."""
import argparse
import contextlib
import hashlib
import io
import json
import os
import re
import subprocess
import sys
import tempfile

HERE = os.path.abspath(__file__)
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(HERE)))
CHILD_TIMEOUT_S = 420
N, BATCH, EPOCHS, CLASSES = 14, 4, 2, 10


def _sha(data):
    return hashlib.sha256(data).hexdigest()


def _state_sha(model):
    import torch
    h = hashlib.sha256()
    for _, v in model.state_dict().items():
        h.update(v.detach().cpu().contiguous().reshape(-1).view(torch.uint8).numpy().tobytes())
    return h.hexdigest()


def _files(top):
    out = []
    for d, _, names in os.walk(top):
        for n in names:
            p = os.path.join(d, n)
            with open(p, "rb") as f:
                out.append([os.path.relpath(p, top), _sha(f.read())])
    return sorted(out)


# ---- the child: one configuration ------------------------------------------------------------------------------------------
def _datasets(torch, np):
    from torch.utils.data import Dataset, TensorDataset

    def gen(seed):
        return torch.Generator().manual_seed(seed)

    class Ragged(Dataset):
        """Decoded images (uint8 [h, w, 3]) of any size with a label."""

        def __init__(self, n, seed):
            rng = np.random.default_rng(seed)
            self.items = [(rng.integers(0, 256, (int(rng.integers(40, 80)), int(rng.integers(40, 80)), 3), dtype=np.uint8),
                           int(rng.integers(0, CLASSES))) for _ in range(n)]

        def __len__(self):
            return len(self.items)

        def __getitem__(self, i):
            return self.items[i]

    def floats(n, S, seed=7, scale=1.0):
        g = gen(seed)
        return TensorDataset(torch.randn(n, 3, S, S, generator=g) * scale, torch.randint(0, CLASSES, (n,), generator=g))

    def u8(n, S, seed=7):
        g = gen(seed)
        return TensorDataset(torch.randint(0, 256, (n, 3, S, S), generator=g, dtype=torch.uint8),
                             torch.randint(0, CLASSES, (n,), generator=g))
    return floats, u8, Ragged


def _configs(gpu):
    """name -> (model name, list of train() keyword builders); a builder takes the toolbox `t` and returns the keywords
    of one train() call.  More than one builder: the calls run one after the other in one output directory."""
    cls = "tiny32_cls"
    c = {
        "cls_eager": (cls, [lambda t: dict(optimizer="fused", dataset=t.floats(N, 32), checkpoint_path="out/model.pth",
                                           selfcheck="raise")]),
        "cls_torch": (cls, [lambda t: dict(optimizer="torch", scheduler=False, dataset=t.floats(N, 32))]),
        "accum_groups_perstep": (cls, [lambda t: dict(optimizer="fused", dataset=t.floats(N, 32), accumulate=3,
                                                      param_groups="no_decay", scheduler_step="step")]),
        "snapshot_then_resume": (cls, [
            lambda t: dict(optimizer="fused", dataset=t.floats(N, 32), snapshot_path="out/run.snap", snapshot_every=2,
                           max_steps=6, ema=0.9),
            lambda t: dict(optimizer="fused", dataset=t.floats(N, 32), snapshot_path="out/run.snap", snapshot_every=2,
                           resume="out/run.snap", ema=0.9)]),
    }
    if not gpu:
        c["reg_val_samples"] = ("nano48_gen", [lambda t: dict(
            optimizer="torch", dataset=t.floats(N, 48, scale=0.5), task="reg", samples_dir="out/samples",
            val_dataset=t.floats(5, 48, seed=9, scale=0.5), checkpoint_path="out/model_reg.pth", ema=0.9)])
        c["distill_accum"] = (cls, [lambda t: dict(optimizer="fused", dataset=t.floats(10, 32), teacher=t.teacher(),
                                                   distill={"mode": "hard"}, accumulate=2)])
        c["cls_eager_2rank"] = c["cls_eager"]
        return c
    c.update({
        "cls_graph_metrics": (cls, [lambda t: dict(optimizer="fused", dataset=t.floats(N, 32), graph=True, device_metrics=True,
                                                   loss_kernels=True)]),
        "collate_aug_crop": (cls, [lambda t: dict(optimizer="fused", dataset=t.u8(N, 36), device_collate=True,
                                                  device_augment=True, crop=(32, 32))]),
        "resize_window": (cls, [lambda t: dict(optimizer="fused", dataset=t.Ragged(N, 3), device_collate=True,
                                               device_resize=(36, 36), crop=(32, 32), resize_window=True)]),
        "random_resized_crop": (cls, [lambda t: dict(
            optimizer="fused", dataset=t.Ragged(N, 3), device_collate=True,
            random_resized_crop=t.trainer.DeviceResizedCrop.random_resized(size=(32, 32), seed=2006))]),
        "reg_collate_val_samples": ("nano48_gen", [lambda t: dict(
            optimizer="fused", dataset=t.u8(N, 52), task="reg", device_collate=True, crop=(48, 48),
            samples_dir="out/samples", val_dataset=t.floats(5, 48, seed=9, scale=0.5), checkpoint_path="out/model_reg.pth",
            ema=0.9, loss_kernels=True)]),
        "distill_graph_accum": (cls, [lambda t: dict(optimizer="fused", dataset=t.floats(10, 32), teacher=t.teacher(),
                                                     distill={"mode": "hard", "graph": True}, accumulate=2)]),
        "val_ema_transform": (cls, [lambda t: dict(
            optimizer="fused", dataset=t.floats(N, 32), val_dataset=t.Ragged(6, 5),
            val_transform=t.trainer.DeviceResizedCrop.center(36, (32, 32)), ema=0.9, val_every=1,
            checkpoint_path="out/model.pth")]),
    })
    return c


def _run_config(name, gpu, rank=0, world=1):
    """-> the JSON records of one configuration (one per train() call), run in the current directory."""
    import numpy as np
    import torch
    import calm_vit_dte_amd as calm
    from importlib import import_module
    from test_host_logic_cpu import build_model
    from helpers import load_golden
    trainer = import_module("calm_vit_dte_amd.trainer")

    class t:
        pass
    t.trainer = trainer
    t.floats, t.u8, t.Ragged = _datasets(torch, np)

    def model(model_name, seed):
        torch.manual_seed(seed)
        if gpu:
            torch.cuda.manual_seed(seed)
        return build_model(model_name, load_golden(model_name) if gpu else None, "cpu").train()
    t.teacher = lambda: model("tiny32_cls", 77).train()
    model_name, builders = _configs(gpu)[name]
    if gpu:
        backend = contextlib.nullcontext()
    else:
        import emulated_recon
        backend = calm.backend.use_backend(emulated_recon.EmulatedReconBackend())
    torch.set_num_threads(2)
    records = []
    with backend:
        for k, make_kw in enumerate(builders):
            m = model(model_name, 50 + 10 * k + rank)          # a resumed run starts elsewhere: only the load makes it equal
            kw = make_kw(t)
            calm.backend.set_loss_kernels(bool(kw.pop("loss_kernels", False)))
            opt = kw.pop("optimizer")
            opt = trainer.make_optimizer(m) if opt == "torch" else opt
            text = io.StringIO()
            with contextlib.redirect_stdout(text):
                out = trainer.train(m, opt, kw.pop("scheduler", None), use_gpu=gpu, epochs=EPOCHS, batch_size=BATCH,
                                    num_classes=CLASSES, log_every=1, **{"selfcheck": None, **kw})
            tag = name + (f"/call{k}" if len(builders) > 1 else "") + (f"/rank{rank}" if world > 1 else "")
            records.append({"name": tag, "stdout": text.getvalue().splitlines(), "state_sha256": _state_sha(out),
                            "files": _files("out") if os.path.isdir("out") else []})
    return records


def _rank_worker(rank, world, port, name):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world),
                      LOCAL_RANK=str(rank))
    with open(f"records{rank}.json", "w") as f:
        json.dump(_run_config(name, False, rank, world), f)


def _child(name, gpu, tree):
    for p in (os.path.join(tree, "tests", "golden"), os.path.join(tree, "tests"), tree):
        sys.path.insert(0, p)
    if name.endswith("_2rank"):
        import socket
        import torch.multiprocessing as mp
        with socket.socket() as s:
            s.bind(("127.0.0.1", 0))
            port = s.getsockname()[1]
        mp.spawn(_rank_worker, args=(2, port, name), nprocs=2, join=True)
        records = [r for rank in range(2) for r in json.load(open(f"records{rank}.json"))]
        for r in records:                                   # the ranks share the directory: its final content
            r["files"] = _files("out")
    else:
        records = _run_config(name, gpu)
    with open("records.json", "w") as f:
        json.dump(records, f)


# ---- the parent: the matrix ------------------------------------------------------------------------------------------------
def _matrix(device, out, tree, only):
    gpu = device == "gpu"
    names = [n for n in _configs(gpu) if not only or n in only]
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, "w") as log:
        for name in names:
            with tempfile.TemporaryDirectory() as work:
                cmd = ["timeout", "-k", "10", str(CHILD_TIMEOUT_S), sys.executable, HERE, "--child", name, "--device", device,
                       "--tree", tree]
                done = subprocess.run(cmd, cwd=work, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
                if done.returncode != 0:
                    print(done.stdout[-4000:])
                    print(f"train_ab: {name} failed with exit status {done.returncode}; stopping", flush=True)
                    return done.returncode
                for rec in json.load(open(os.path.join(work, "records.json"))):
                    log.write(json.dumps(rec) + "\n")
                    log.flush()
            print(f"train_ab: {name} done", flush=True)
    return 0


_NUMBER = re.compile(r"[-+]?(?:\d+\.?\d*(?:[eE][-+]?\d+)?|nan|inf)")


def _compare(a, b, masked):
    ra = [json.loads(line) for line in open(a)]
    rb = [json.loads(line) for line in open(b)]
    bad = [] if [r["name"] for r in ra] == [r["name"] for r in rb] else ["the runs' names differ"]
    for x, y in zip(ra, rb):
        if x["name"].split("/")[0] in masked:
            x, y = ({"name": r["name"], "stdout": [_NUMBER.sub("#", s) for s in r["stdout"]],
                     "files": [f[0] for f in r["files"]]} for r in (x, y))
        for field in x:
            if x[field] != y[field]:
                bad.append(f"{x['name']}: {field} differs")
    print("\n".join(bad) if bad else f"{len(ra)} records agree" + (f" ({', '.join(sorted(masked))} masked)" if masked else ""))
    return 1 if bad else 0


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--device", choices=["cpu", "gpu"], default="cpu")
    ap.add_argument("--out")
    ap.add_argument("--tree", default=ROOT)
    ap.add_argument("--only", default="")
    ap.add_argument("--child")
    ap.add_argument("--compare", nargs=2, metavar=("A", "B"))
    ap.add_argument("--masked", default="")
    args = ap.parse_args()
    split = lambda s: {n for n in s.split(",") if n}
    if args.compare:
        return _compare(*args.compare, split(args.masked))
    tree = os.path.abspath(args.tree)
    if args.child:
        return _child(args.child, args.device == "gpu", tree)
    if not args.out:
        ap.error("--out FILE is needed")
    return _matrix(args.device, args.out, tree, split(args.only))


if __name__ == "__main__":
    sys.exit(main())
