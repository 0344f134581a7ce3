"""fused_samples.SampleSet on its own, without a step and without a GPU: the ray set is a recording fake, `supported` takes
16x32 and 8x16 textures and refuses 4x8, the two traces, shading_ops.build_taps and sampling.fibonacci_sphere_sampling are
recorded.  The generated kind (device visibility: no direction tensor) is covered here and nowhere else on the CPU."""
import math

import pytest
import torch

P, K, M = 7, 8, 16
TWO_PI = float(torch.tensor(2 * math.pi, dtype=torch.float32))


@pytest.fixture
def world(monkeypatch):
    """-> (events, a SampleSet factory, the activated parameters acquire() takes)"""
    from relightable3dgaussian_amd import fused_samples, sampling, shading_ops
    events = []

    class FakeRaySet:
        def __init__(self, normals=None, sample_num=None):
            events.append(("FixedRaySet", normals, sample_num))

        @classmethod
        def try_build(cls, normals, dirs, **k):
            events.append(("try_build", normals, dirs))
            return cls.__new__(cls)

        supported = staticmethod(lambda K_, M_, He, We: (K_, M_) == (K, M) and (He, We) in ((16, 32), (8, 16)))

        def taps(self, He, We):
            events.append(("frs.taps", self, He, We))

    def build_taps(dirs, He, We, *a, **k):
        events.append(("build_taps", dirs, He, We))
        return torch.zeros(P * K * 3)

    real = sampling.fibonacci_sphere_sampling
    monkeypatch.setattr(sampling, "fibonacci_sphere_sampling", lambda n, k: events.append(("fibonacci", n.shape[0], k)) or real(n, k))
    monkeypatch.setattr(shading_ops, "FixedRaySet", FakeRaySet)
    monkeypatch.setattr(shading_ops, "build_taps", build_taps)
    trace = lambda *a, group=None: events.append(("trace", a[5], group)) or (
        torch.ones(P, K, 1), torch.ones(P, K, 3), torch.full((P, K, 1), 2.0), "tracer")
    trace_on_device = lambda *a, group=None, want_dirs=False: events.append(("device trace", a[5], group, want_dirs)) or (
        torch.ones(P, K, 1), torch.ones(P, K, 3) if want_dirs else None, "tracer")
    g = torch.Generator().manual_seed(3)
    normal = torch.nn.functional.normalize(torch.randn(P, 3, generator=g), dim=-1)
    activated = (torch.zeros(P, 3), torch.ones(P, 3), torch.zeros(P, 4), torch.ones(P, 1), normal)
    return events, (lambda **kw: fused_samples.SampleSet(K, M, (trace, trace_on_device), **kw)), activated


def kinds(events):
    return [e[0] for e in events]


def test_generated_kind_selects_builds_materialises_and_refreshes(world):
    events, make, activated = world
    s = make(group="the group", device_visibility=True)
    s.acquire(*activated)
    assert events == [("device trace", K, "the group", False)]
    assert s.incident_dirs is None and s.incident_areas is None and s.tracer == "tracer" and s.visibility.shape == (P, K, 1)
    assert torch.equal(s.ray_normals, activated[4]) and s.ray_normals is not activated[4]          # a snapshot
    # the first selection builds a ray set with no comparison pass
    del events[:]
    assert s.select(16, 32) is None
    assert kinds(events) == ["FixedRaySet", "frs.taps"] and events[0][1] is s.ray_normals and events[0][2] == K
    first = s.frs
    assert first is not None and events[1] == ("frs.taps", first, 16, 32) and s.uniform_area == TWO_PI and s.taps is None
    # the same size again: nothing; another size the kernels take: only new lookup records of the SAME ray set
    del events[:]
    assert s.select(16, 32) is None and events == []
    assert s.select(8, 16) is None and events == [("frs.taps", first, 8, 16)] and s.frs is first
    # a size they refuse: directions and areas come into being, the general path shades, its taps are built from that tensor
    del events[:]
    taps = s.select(4, 8)
    assert kinds(events) == ["fibonacci", "try_build", "build_taps"]
    dirs = s.incident_dirs
    assert taps is s.taps and taps is not None and s.frs is None and s.uniform_area == TWO_PI
    assert dirs.shape == (P, K, 3) and torch.equal(s.incident_areas, torch.full((P, K, 1), TWO_PI))
    assert events[1][1] is s.ray_normals and events[1][2] is dirs and events[2][1] is dirs and events[2][2:] == (4, 8)
    from relightable3dgaussian_amd import sampling
    assert torch.equal(dirs, sampling.fibonacci_directions(s.ray_normals, K)[0])
    # ... and from then on the set is of the stored kind: the ray set try_build made serves the sizes it takes
    del events[:]
    assert s.select(4, 8) is taps and events == []
    assert s.select(16, 32) is None and kinds(events) == ["frs.taps"] and s.frs is not None and s.frs is not first
    # refresh: re-traced on the device, the key moves, everything is rebuilt for the size that was in use
    del events[:]
    moved = tuple(t.clone() for t in activated[:4]) + (-activated[4],)
    s.refresh(*moved)
    assert kinds(events) == ["device trace", "FixedRaySet", "frs.taps"] and events[0][3] is False and events[2][2:] == (16, 32)
    assert s.refreshes == 1 and s.incident_dirs is None and s.incident_areas is None and torch.equal(s.ray_normals, moved[4])
    assert events[1][1] is s.ray_normals and s.frs is events[2][1] and s.taps is None
    del events[:]
    assert s.select(16, 32) is None and events == []
    # release, as the benchmark does it by hand (through the step's forwarding properties): None means "drop it"
    s.visibility = s.incident_dirs = s.incident_areas = None
    s.taps = s.src = s.frs = None
    assert s.visibility is None and s.frs is None and s.taps is None and s.src is None


def test_generated_kind_without_the_fixed_ray_set_kernels_goes_straight_to_tensors(world, monkeypatch):
    events, make, activated = world
    monkeypatch.setenv("R3DG_SHADE_FRS", "0")
    s = make(device_visibility=True)
    s.acquire(*activated)
    assert events == [("device trace", K, None, True)]               # the general kernels will read the directions: traced with them
    assert s.incident_dirs.shape == (P, K, 3) and torch.equal(s.incident_areas, torch.full((P, K, 1), TWO_PI))
    # a set that holds no tensor (dropped from outside) and may not build a ray set: materialise, general path
    s.incident_dirs = s.incident_areas = None
    del events[:]
    taps = s.select(16, 32)
    assert kinds(events) == ["fibonacci", "build_taps"] and taps is not None and s.frs is None and s.uniform_area == TWO_PI
    assert events[1][1] is s.incident_dirs and s.incident_areas.shape == (P, K, 1)


def test_stored_kind_keys_on_the_direction_tensor_and_reads_the_areas(world):
    events, make, activated = world
    s = make()
    s.acquire(*activated)
    assert events == [("trace", K, None)] and s.incident_dirs.shape == (P, K, 3) and s.refreshes == 0
    # uniform areas: one ray set per direction tensor, lookup records per size
    del events[:]
    assert s.select(16, 32) is None and kinds(events) == ["try_build", "frs.taps"] and s.uniform_area == 2.0
    built = s.frs
    assert s.select(8, 16) is None and kinds(events) == ["try_build", "frs.taps", "frs.taps"] and s.frs is built
    # areas that differ: no ray set, every sample's area is read
    s.incident_areas = torch.cat([torch.full((P, K - 1, 1), 2.0), torch.full((P, 1, 1), 3.0)], 1)
    s.incident_dirs = torch.ones(P, K, 3)
    del events[:]
    taps = s.select(16, 32)
    assert kinds(events) == ["build_taps"] and taps is s.taps and s.frs is None and s.uniform_area is None
    # the same tensor edited in place, and another size: each rebuilds the taps; the same key does not
    assert s.select(16, 32) is taps and len(events) == 1
    s.incident_dirs.add_(1.0)
    s.select(16, 32)
    s.select(8, 16)
    assert kinds(events) == ["build_taps"] * 3
    # no tensor, then a tensor again: generated in between (ray set of the snapshot normals), stored afterwards
    s.incident_dirs = None
    del events[:]
    assert s.select(16, 32) is None and kinds(events) == ["FixedRaySet", "frs.taps"] and s.uniform_area == TWO_PI
    s.incident_dirs, s.incident_areas = torch.ones(P, K, 3), torch.full((P, K, 1), 2.0)
    del events[:]
    assert s.select(16, 32) is None and kinds(events) == ["try_build", "frs.taps"] and events[0][2] is s.incident_dirs
    assert s.uniform_area == 2.0 and s.src is s.incident_dirs
    # refresh is the device trace whichever way the set was acquired
    del events[:]
    s.refresh(*activated)
    assert kinds(events) == ["device trace", "FixedRaySet", "frs.taps"] and s.refreshes == 1 and s.incident_dirs is None
