"""
Records what Learner's constructor decides for a table of shapes -> tests/golden/chain_plan.json, on a machine without a GPU.

Usage:  python tests/golden/make_chain_plan.py          (writes tests/golden/chain_plan.json of the tree the script stands in)

The committed file was written by this script standing in a checkout of the commit BEFORE chain_plan.py existed (NOTEBOOK.md names
it): it is what that constructor chose, and tests/test_chain_plan_cpu.py holds plan_chain() to it. Run on a later tree it must
reproduce the file byte for byte — that is the check that Learner still carries what the plan says. It therefore reads only
attributes and buffer shapes that both trees have.

How the learner is constructed without a GPU: _lib.require_gpu replaced by a no-op, torch.Tensor.pin_memory by the identity,
NAF_BLAS_DEFAULT=1 (torch's BLAS settings untouched), device "cpu", world_size 1.

Format (3,362 cases must stay under 512 KB; half of them warn, with texts of 250 bytes): one row per case in "cases" —
[S, A, H, B, p_mode, variant, choice, norm, batch]; the last four are indices into the tables of the same names, which hold every
DISTINCT tuple of their columns once ("columns" names them). A warning text is stored with the case's own S, A, H, B written as
{S}, {A}, {H}, {B} where putting the numbers back gives the text exactly (checked here; the text itself otherwise).
"""
import itertools
import json
import os
import re
import sys
import warnings

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
os.environ["NAF_BLAS_DEFAULT"] = "1"
for _k in ("NAF_FUSE", "NAF_DEFER_ADAM"):
    os.environ.pop(_k, None)

import torch  # noqa: E402

from robotic_manipulator_rloa_amd import _lib  # noqa: E402

_lib.require_gpu = lambda: None
torch.Tensor.pin_memory = lambda self, *a, **k: self

from robotic_manipulator_rloa_amd.learner import Learner  # noqa: E402

# what a case varies besides the shape: keyword arguments of Learner and environment switches
VARIANTS = [{}] + [{"fuse": c} for c in ("rows", "columns", "unfused")] + \
    [{"env": {"NAF_FUSE": c}} for c in ("rows", "columns", "unfused")] + \
    [{"pad_layer": False}, {"_fold_norm": False}, {"_force_allreduce": True}, {"env": {"NAF_DEFER_ADAM": "0"}}, {"fuse": "tiles"}]
BASES = [(21, 6, 256, 256), (23, 7, 256, 2048), (27, 9, 256, 2048), (27, 9, 256, 4096), (21, 6, 512, 300), (40, 4, 256, 32),
         (21, 6, 128, 64), (21, 6, 256, 15), (11, 1, 256, 48), (21, 6, 256, 20000)]
COLUMNS = {
    "choice": ["chain", "fuse", "bb_ok", "fold_norm", "defer_ok", "keep_xhat1", "warnings", "error"],
    "norm": ["n_partials", "n_partials_fold", "n_partials_norm", "partials_numel", "gb_blocks", "gb_wh_blocks", "ft_blocks",
             "mom_floats"],
    "batch": ["Bp", "n_loss_wg", "hk_rows", "nb1", "ks_w2", "ks_wh", "exchange_floats", "n_slabs", "slab_stride"],
}


def cases():
    """[S, A, H, B, p_mode, variant]: the full product at the defaults, one factor at a time from each base, the errors."""
    out = [list(c) + [0] for c in itertools.product((21, 24, 25, 32, 33), (6, 8, 9, 11, 12), (128, 256, 384, 512, 513),
                                                    (15, 16, 64, 256, 257, 512, 513, 1000, 1024, 2048, 2049, 4096, 4097), (0, 1))]
    out += [list(b) + [0, v] for b in BASES for v in range(len(VARIANTS) - 1)]
    out += [[21, 6, 256, 0, 0, 0], [21, 6, 256, 2 ** 20 + 1, 0, 0], [21, 6, 256, 256, 0, len(VARIANTS) - 1],
            [21, 0, 256, 256, 0, 0], [21, 65, 256, 256, 0, 0]]
    seen, unique = set(), []
    for c in out:
        if tuple(c) not in seen:
            seen.add(tuple(c))
            unique.append(c)
    return unique


def templated(text, S, A, H, B):
    if "{" in text or "}" in text:
        return text
    t = text
    for name, v in (("B", B), ("S", S), ("H", H), ("A", A)):
        t = re.sub(rf"\b{v}\b", "{" + name + "}", t)
    return t if t.format(S=S, A=A, H=H, B=B) == text else text


def record(S, A, H, B, p_mode, variant):
    """the learner's choices for one case, by column"""
    kw = {k: v for k, v in VARIANTS[variant].items() if k != "env"}
    env = VARIANTS[variant].get("env", {})
    os.environ.update(env)
    try:
        with warnings.catch_warnings(record=True) as caught:
            warnings.simplefilter("always")
            try:
                L = Learner(S, A, H, B, 1e-3, 1e-3, 0.99, "cpu", p_mode=p_mode, **kw)
            except ValueError as e:
                return {"error": str(e)}
    finally:
        for k in env:
            del os.environ[k]
    bb = hasattr(L, "bb_slab_w2")
    exchange = getattr(L, "bb_exchange", None)
    return {
        "chain": L.chain, "fuse": ",".join(sorted(L.fuse)), "bb_ok": L.bb_ok, "fold_norm": L.fold_norm, "defer_ok": L.defer_ok,
        "keep_xhat1": torch.is_tensor(getattr(L, "XH1", None)), "warnings": [templated(str(w.message), S, A, H, B) for w in caught],
        "error": None,
        "n_partials": L.n_partials, "n_partials_fold": L.n_partials_fold, "n_partials_norm": L.n_partials_norm,
        "partials_numel": L.partials.numel(), "gb_blocks": L._gb_blocks, "gb_wh_blocks": L._gb_wh_blocks, "ft_blocks": L._ft_blocks,
        "mom_floats": getattr(L, "mom_floats", None),
        "Bp": L.Bp, "n_loss_wg": L.n_loss_wg, "hk_rows": getattr(L, "hk_rows", None), "nb1": getattr(L, "_nb1", None),
        "ks_w2": L.bb_slab_w2.shape[0] if bb else None, "ks_wh": L.bb_slab_wh.shape[0] if bb else None,
        "exchange_floats": exchange.numel() if exchange is not None else None,
        "n_slabs": getattr(L, "n_slabs", None), "slab_stride": getattr(L, "slab_stride", None),
    }


def main():
    tables = {g: [] for g in COLUMNS}
    index = {g: {} for g in COLUMNS}
    rows = []
    for case in cases():
        got = record(*case)
        row = list(case)
        for g, cols in COLUMNS.items():
            tup = [got.get(c) for c in cols]
            key = json.dumps(tup)
            if key not in index[g]:
                index[g][key] = len(tables[g])
                tables[g].append(tup)
            row.append(index[g][key])
        rows.append(row)
    dump = lambda x: json.dumps(x, separators=(",", ":"))          # noqa: E731
    lines = ['{"case_columns":' + dump(["S", "A", "H", "B", "p_mode", "variant"] + list(COLUMNS)) + ",",
             '"variants":' + dump(VARIANTS) + ",", '"columns":' + dump(COLUMNS) + ","]
    for g in COLUMNS:
        lines.append(f'"{g}":[\n' + ",\n".join(dump(t) for t in tables[g]) + "],")
    lines.append('"cases":[\n' + ",\n".join(dump(r) for r in rows) + "]}")
    path = os.path.join(HERE, "chain_plan.json")
    with open(path, "w") as f:
        f.write("\n".join(lines) + "\n")
    print(f"{path}: {len(rows)} cases, " + ", ".join(f"{len(tables[g])} {g}" for g in COLUMNS) + f", {os.path.getsize(path)} bytes")


if __name__ == "__main__":
    main()
