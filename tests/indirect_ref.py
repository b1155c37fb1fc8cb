"""The indirect surface draw (sailor_amd/csrc/surface_indirect.hip) restated from the rules pinned in include/sailor_hip.h, on top of the existing sequential
restatements (tests/surface_ref.py, tests/masked_ref.py, tests/gltf_ref.py).

A scene is surface_ref's dict.  A draw that carries `indirect=dict(capacity=, count=, first=, records=)` is one command of DrawIndexedIndirect: capacity is
the instanceCount the host wrote, count and first are the instanceCount and firstInstance the command holds when the draw RUNS, records is the
numInstanceRecords of the call (None: the scene's `records`).  Its instance_ids / num_drawn / first_instance are not read.  The scene's `instances` may hold
more records than `records` says (slack that no draw may reach).

  drawn(ind, records)     rule 3: n = min(count, capacity, records - first), 0 when first >= records
  survivors(scene)        the DIRECT scene of the same picture: every indirect draw replaced by a draw of num_drawn = n from first_instance = first
  expected(scene, ...)    the existing restatement on survivors(scene): what the picture must be
  prim_table(scene, how)  per draw (primBase, extent, numTriangles, n): how="capacity" advances as the indirect pass does (rule 5), "survivors" as the direct one
  decode(keys, table)     a key's owner as (slot, d, triangle, part) by its side's own table, and the depth bits
  render_keys(scene, ...) the indirect pass's OWN keys, formed as the kernels form them: every draw on its own against the pass's starting depth, with its
                          capacity-based primBase, and the unsigned maximum of the keys -- no draw sees another one's depth.  That this decodes to the owners
                          of the sequential survivors pass is the invariant tests/test_indirect_cpu.py holds for every case."""
import numpy as np

import gltf_ref
import masked_ref

LOW = np.uint64(0xFFFFFFFF)


def drawn(ind, records):
    records = records if ind.get("records") is None else int(ind["records"])
    first, count, capacity = int(ind["first"]), int(ind["count"]), int(ind["capacity"])
    room = records - first if first < records else 0
    return min(count, capacity, room)


def _records(scene):
    return int(scene["records"]) if scene.get("records") is not None else len(scene["instances"])


def _direct_count(scene, d):
    if d.get("num_drawn") is not None:
        return int(d["num_drawn"])
    return len(d["instance_ids"]) if d.get("instance_ids") is not None else len(scene["instances"]) - int(d.get("first_instance", 0))


def survivors(scene):
    out = dict(scene)
    draws = []
    for d in scene["draws"]:
        ind = d.get("indirect")
        if ind is None:
            draws.append(d)
            continue
        n = drawn(ind, _records(scene))
        e = dict(d, instance_ids=None, num_drawn=n, first_instance=int(ind["first"]) if n else 0)
        del e["indirect"]
        draws.append(e)
    out["draws"] = draws
    return out


def renderer(scene):
    return gltf_ref.render if any(d.get("gltf", False) for d in scene["draws"]) else masked_ref.render


def expected(scene, prepass=None, rows=None):
    s = survivors(scene)
    return renderer(s)(s, prepass=prepass, rows=rows)


def prim_table(scene, how):
    assert how in ("capacity", "survivors")
    table, base = [], int(scene.get("prim_base", 0))
    for d in scene["draws"]:
        nt, ind = len(np.asarray(d["indices"]).reshape(-1, 3)), d.get("indirect")
        n = drawn(ind, _records(scene)) if ind is not None else _direct_count(scene, d)
        advance = int(ind["capacity"]) if (ind is not None and how == "capacity") else n
        table.append((base, advance * 2 * nt, nt, n))
        base += advance * 2 * nt
    return table


def decode(keys, table):
    """-> dict(slot, d, triangle, part: int64 arrays, -1 where no primitive owns the pixel; depth: the keys' high words).  Every owned pixel must fall into
    exactly one draw's range and name an instance below that draw's n."""
    keys = np.asarray(keys, np.uint64)
    low = (keys & LOW).astype(np.int64)
    order = low - 1
    slot, d, tri, part = (np.full(keys.shape, -1, np.int64) for _ in range(4))
    for k, (base, extent, nt, n) in enumerate(table):
        m = (low > 0) & (order >= base) & (order < base + extent)
        if not m.any():
            continue
        assert (slot[m] == -1).all(), f"draw {k}: its range overlaps an earlier one"
        rel = order[m] - base
        slot[m], d[m], tri[m], part[m] = k, rel // (2 * nt), (rel % (2 * nt)) // 2, rel & 1
        assert (d[m] < n).all(), f"draw {k}: a key names instance {int(d[m].max())} of {n} drawn"
    assert ((low > 0) == (slot >= 0)).all(), "a key belongs to no draw of the table"
    return dict(slot=slot, d=d, triangle=tri, part=part, depth=(keys >> np.uint64(32)).astype(np.uint32))


def same_owners(a, b):
    return all(np.array_equal(a[k], b[k]) for k in ("slot", "d", "triangle", "part", "depth"))


def render_keys(scene, prepass=None, rows=None):
    s = survivors(scene)
    render = renderer(s)
    H, W = scene["H"], scene["W"]
    r0, r1 = rows if rows is not None else (0, H)
    start = np.zeros((H, W), np.float32) if prepass is None else np.asarray(prepass, np.float32).reshape(H, W)
    keys = start[r0:r1].view(np.uint32).astype(np.uint64) << np.uint64(32)
    for d, (base, _, _, n) in zip(s["draws"], prim_table(scene, "capacity")):
        if n == 0 or len(np.asarray(d["indices"]).reshape(-1, 3)) == 0:
            continue
        alone = dict(s, draws=[d], prim_base=base)
        keys = np.maximum(keys, render(alone, prepass=prepass, rows=rows)["keys"])
    return keys
