"""The public surface of qdsp_amd.ops, pinned line by line to tests/golden/ops_surface.txt: every public class and function the
module defines, every public attribute of each class (inherited ones included) with its signature, every upper-case constant with
its value, and `__all__`.  A method that appears, vanishes, moves between instance / class / static, or changes a default shows
as a differing line.  Needs no library: importing `ops` loads nothing.

`python tests/test_ops_surface_cpu.py --write` regenerates the file; do that only when the surface is meant to change."""
import inspect
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
GOLDEN = os.path.join(ROOT, "tests", "golden", "ops_surface.txt")


def _sig(obj) -> str:
    return str(inspect.signature(obj))


def surface_lines():
    from qdsp_amd import ops

    lines = [f"__all__ = {list(ops.__all__)!r}"]
    for name, obj in sorted(vars(ops).items()):
        if name.startswith("_") or getattr(obj, "__module__", None) != ops.__name__:
            continue
        if inspect.isfunction(obj):
            lines.append(f"{name}{_sig(obj)}")
        elif inspect.isclass(obj):
            lines.append(f"{name}{_sig(obj)}")                       # the constructor, as a caller writes it
            for attr in sorted(dir(obj)):
                if attr.startswith("_"):
                    continue
                raw, val = inspect.getattr_static(obj, attr), getattr(obj, attr)
                if isinstance(raw, property):
                    lines.append(f"{name}.{attr} <property>")
                elif callable(val):
                    tag = {staticmethod: " <static>", classmethod: " <classmethod>"}.get(type(raw), "")
                    lines.append(f"{name}.{attr}{_sig(val)}{tag}")
                elif attr.isupper():
                    lines.append(f"{name}.{attr} = {val!r}")
                else:
                    lines.append(f"{name}.{attr}")
    return lines


def test_public_surface_is_the_recorded_one():
    with open(GOLDEN) as f:
        want = f.read().splitlines()
    got = surface_lines()
    gone, new = [l for l in want if l not in got], [l for l in got if l not in want]
    assert got == want, "qdsp_amd.ops's public surface moved:\n" + "\n".join(["- " + l for l in gone] + ["+ " + l for l in new])


if __name__ == "__main__":
    if sys.argv[1:] == ["--write"]:
        with open(GOLDEN, "w") as f:
            f.write("\n".join(surface_lines()) + "\n")
        print(f"wrote {GOLDEN}")
    else:
        sys.exit("usage: test_ops_surface_cpu.py --write")
