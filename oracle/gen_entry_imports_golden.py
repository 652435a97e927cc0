"""Record the import graph the reference's entry scripts walk -- build container only:

    python oracle/gen_entry_imports_golden.py        ->  tests/golden/entry_script_imports.json

For each entry script (train/eval x AVA/JHMDB): the import statements of its import block (everything before the first ``def``), as
[module, [names]] (``from module import names``) or [module, null] (``import module``).  For every module of the reference's own
packages that those statements reach and this repository does NOT provide (``utils.utils``, ``datasets.ava_frame`` ...), transitively:
whether it is a package, the statements of the same form by which it imports from the reference's packages (``datasets.ava_frame``
takes ``collate_fn`` from ``utils.misc``, which this repository serves), and the names others take from it.  Module names and
imported names only: no code of the reference.  tests/test_cpu.py stands stub modules with these imports up on a second sys.path
entry, so the drop-in packages' path extension is exercised exactly as with the reference checkout behind this repository.
"""
import ast
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from oracle import ref_import  # noqa: E402

SCRIPTS = ("train_tuber_ava.py", "eval_tuber_ava.py", "train_tuber_jhmdb.py", "eval_tuber_jhmdb.py")


def _path(base, mod):
    """(file, is_package) of module ``mod`` under ``base``, or None"""
    p = os.path.join(base, *mod.split("."))
    if os.path.isfile(os.path.join(p, "__init__.py")):
        return os.path.join(p, "__init__.py"), True
    if os.path.isfile(p + ".py"):
        return p + ".py", False
    return None


def _statements(tree, mod=None, is_pkg=False):
    """[[module, [names]] | [module, None]] of the top-level imports of ``tree`` (relative imports made absolute)"""
    out = []
    for node in tree.body:
        if isinstance(node, ast.Import):
            out += [[a.name, None] for a in node.names]
        elif isinstance(node, ast.ImportFrom):
            name = node.module or ""
            if node.level:
                parts = mod.split(".")[:len(mod.split(".")) - node.level + (1 if is_pkg else 0)]
                name = ".".join(parts + ([name] if name else []))
            out.append([name, [a.name for a in node.names]])
    return out


def main():
    assert ref_import.available(), "needs the reference checkout"
    ref = ref_import.REF
    tops = {d for d in os.listdir(ref) if os.path.isfile(os.path.join(ref, d, "__init__.py"))}
    scripts, modules, queue = {}, {}, []

    def reach(stmts):
        for m, names in stmts:
            if m.split(".")[0] not in tops:
                continue
            cands = [m] + [m + "." + n for n in (names or []) if _path(ref, m + "." + n)]
            parts = m.split(".")
            cands += [".".join(parts[:i]) for i in range(1, len(parts))]            # parent packages are imported too
            for c in cands:
                if _path(ROOT, c) is None and _path(ref, c) is not None and c not in modules:
                    modules[c] = None
                    queue.append(c)
            if names and _path(ROOT, m) is None and _path(ref, m) is not None:
                exports = modules.setdefault("__exports__", {}).setdefault(m, set())
                exports.update(n for n in names if not _path(ref, m + "." + n))

    for s in SCRIPTS:
        src = open(os.path.join(ref, s)).read()
        block = src[:src.index("\ndef ")] if "\ndef " in src else src
        scripts[s] = _statements(ast.parse(block))
        reach(scripts[s])
    while queue:
        m = queue.pop(0)
        path, is_pkg = _path(ref, m)
        stmts = [st for st in _statements(ast.parse(open(path).read()), m, is_pkg) if st[0].split(".")[0] in tops]
        modules[m] = {"package": is_pkg, "imports": stmts}
        reach(stmts)
    exports = modules.pop("__exports__", {})
    for m, rec in modules.items():
        rec["exports"] = sorted(exports.get(m, ()))
    out = {"packages": sorted(tops), "scripts": scripts, "modules": dict(sorted(modules.items())),
           "generator": "oracle/gen_entry_imports_golden.py (ast of the reference's entry scripts and the modules they reach)"}
    dst = os.path.join(ROOT, "tests", "golden", "entry_script_imports.json")
    with open(dst, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print("%d scripts, %d reference modules this repository does not provide -> %s" % (len(scripts), len(modules), dst))


if __name__ == "__main__":
    main()
