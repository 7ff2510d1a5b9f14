"""build_hip()'s dependency list (hip_sources) against what mdstep.hip really includes: host logic only."""
import os
import re

import __graft_entry__ as entry

INCLUDE = re.compile(r'^\s*#\s*include\s+"([^"]+)"', re.M)


def reachable_includes():
    """[(including file, included file)] for every #include "..." reachable from mdstep.hip, resolved like the compiler does:
    beside the including file first, then under include/ (-Iinclude)."""
    root = entry.hip_sources()[0]
    edges, todo, seen = [], [root], {root}
    while todo:
        f = todo.pop()
        for name in INCLUDE.findall(open(f).read()):
            tries = [os.path.join(os.path.dirname(f), name), os.path.join(entry.ROOT, "include", name)]
            hit = next((os.path.normpath(t) for t in tries if os.path.isfile(t)), None)
            assert hit, "%s includes %s, which is neither beside it nor under include/" % (f, name)
            edges.append((f, hit))
            if hit not in seen:
                seen.add(hit)
                todo.append(hit)
    return edges


def test_every_reachable_include_is_a_build_dependency():
    sources = set(entry.hip_sources())
    assert all(os.path.isfile(s) for s in sources)
    missing = sorted({hit for _, hit in reachable_includes()} - sources)
    assert not missing, "build_hip() would keep a stale library after an edit to %s" % missing


def test_every_part_is_included_exactly_once():
    parts_dir = os.path.join(os.path.dirname(entry.hip_sources()[0]), "parts")
    parts = sorted(os.path.join(parts_dir, f) for f in os.listdir(parts_dir) if f.endswith(".inc"))
    assert parts and set(parts) <= set(entry.hip_sources())
    included = [hit for _, hit in reachable_includes() if os.path.dirname(hit) == parts_dir]
    assert sorted(included) == parts


def test_every_part_names_itself_in_its_first_line():
    parts = [s for s in entry.hip_sources() if s.endswith(".inc")]
    assert parts
    for p in parts:
        first = open(p).readline()
        assert first.startswith("// parts/%s -- part of mdstep.hip" % os.path.basename(p)), p
