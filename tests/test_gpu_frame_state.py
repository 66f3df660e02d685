"""The frame slot's scheduling state, frame by frame, as the library itself reports it.

Pixels never depend on the scheduling feedback, so no parity test can see a launch order that is no longer kept, costs that are
collected for ever, or a slot that forgets to start afresh.  GRT_DEBUG_LAUNCH=1 makes every launch print one line to stderr,

    grt launch: ctx P mode M units U order yes|no entries E cost collect|- parts_ok B cost_valid B order_ready B used . thr4 . max .

and this test runs one scripted sequence of frames in a fresh child process (the switch is read once per process) and compares the
host-side fields of every line — everything up to `used`, which starts what the ordering kernel left on the device — with EXPECTED.

EXPECTED was recorded from the library as it was BEFORE the frame launch moved into a unit of its own (csrc/grt_frame.hip), not from a
reading of the code, and the test passes unchanged on that library and on this one.  Where the record disagrees with what one would
expect from the comments in the code, the record is right.  What it shows, step by step (SCRIPT below):

  standing   frame 1 is cold: an estimated order with parts (entries = units + parts_extra_cap = 4096) and costs collected; frame 2 runs with
             the order made behind frame 1 and collects again (an order made from costs measured under the cold order's parts is used
             but not kept); from frame 3 on the order is kept and nothing is collected: `cost -`, order_ready 1, the same `entries`,
             frame after frame.  (Two collecting frames, not three.)
  move       another eye: the order in hand is used, and costs are collected for two frames again
  window     a 128x128 window is another launch geometry: 256 units, cold
  tiles      grt_render_tiles has units and a signature of its own (mode 1, 512 units): its cold order has no parts (entries 0), the
             order made behind the first frame has
  rays       grt_render_rays, 4096 rays: mode 2, 16 units, parts_ok 0, never an order with parts; the first frame has no order and
             collects, the second has one and keeps it
  option     GRT_OPT_TILE_PARTS4_PCT on a settled view invalidates the costs: the next frame is cold again
  feedback0  GRT_OPT_FEEDBACK 0: `order no`, but the tile kernel's cost words are still collected (for the give-up check), cost_valid 0;
             with the feedback back on the next frame is cold
  upload     a new upload (scene epoch) resets the slot: cold
  view       a view rendering on a side stream has state of its own (slot 1): cold, collecting, kept — while its parent's slot, asked
             for a frame afterwards, is as settled as it was
  aux_mesh   a scene with meshes: the cold order has no parts (entries 0).  The third frame is an aux frame, which runs on the per-lane
             kernel; its line is printed before it drops its order and shows the kept one, and the plain frame behind it starts the
             feedback afresh: cold, where a fourth plain frame would have printed `cost -`
"""
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N, W, H = 20000, 256, 256  # 1024 tiles: under three times the resident waves, so the quad-parts path is live

# (step, frames): what the child runs, in this order; every frame is waited for before the next one is launched
SCRIPT = (("standing", 6), ("move", 4), ("window", 2), ("tiles", 2), ("rays", 2), ("option", 3), ("feedback0", 3), ("upload", 2),
          ("view", 4), ("aux_mesh", 5))

# per step, per frame: (slot, mode, units, order, entries, cost, parts_ok, cost_valid, order_ready); slot = contexts in the order they first print
EXPECTED = {
    "standing": [
        (0, 0, 1024, 'yes', 4096, 'collect', 1, 1, 0),
        (0, 0, 1024, 'yes', 4096, 'collect', 1, 1, 0),
        (0, 0, 1024, 'yes', 4096, '-', 1, 1, 1),
        (0, 0, 1024, 'yes', 4096, '-', 1, 1, 1),
        (0, 0, 1024, 'yes', 4096, '-', 1, 1, 1),
        (0, 0, 1024, 'yes', 4096, '-', 1, 1, 1),
    ],
    "move": [
        (0, 0, 1024, 'yes', 4096, 'collect', 1, 1, 0),
        (0, 0, 1024, 'yes', 4096, 'collect', 1, 1, 0),
        (0, 0, 1024, 'yes', 4096, '-', 1, 1, 1),
        (0, 0, 1024, 'yes', 4096, '-', 1, 1, 1),
    ],
    "window": [
        (0, 0, 256, 'yes', 1024, 'collect', 1, 1, 0),
        (0, 0, 256, 'yes', 1024, 'collect', 1, 1, 0),
    ],
    "tiles": [
        (0, 1, 512, 'yes', 0, 'collect', 1, 1, 0),
        (0, 1, 512, 'yes', 2048, 'collect', 1, 1, 0),
    ],
    "rays": [
        (0, 2, 16, 'no', 0, 'collect', 0, 1, 0),
        (0, 2, 16, 'yes', 0, '-', 0, 1, 1),
    ],
    "option": [
        (0, 0, 1024, 'yes', 4096, 'collect', 1, 1, 0),
        (0, 0, 1024, 'yes', 4096, 'collect', 1, 1, 0),
        (0, 0, 1024, 'yes', 4096, '-', 1, 1, 1),
    ],
    "feedback0": [
        (0, 0, 1024, 'no', 0, 'collect', 1, 0, 0),
        (0, 0, 1024, 'no', 0, 'collect', 1, 0, 0),
        (0, 0, 1024, 'yes', 4096, 'collect', 1, 1, 0),
    ],
    "upload": [
        (0, 0, 1024, 'yes', 4096, 'collect', 1, 1, 0),
        (0, 0, 1024, 'yes', 4096, 'collect', 1, 1, 0),
    ],
    "view": [
        (1, 0, 1024, 'yes', 4096, 'collect', 1, 1, 0),
        (1, 0, 1024, 'yes', 4096, 'collect', 1, 1, 0),
        (1, 0, 1024, 'yes', 4096, '-', 1, 1, 1),
        (0, 0, 1024, 'yes', 4096, '-', 1, 1, 1),
    ],
    "aux_mesh": [
        (0, 0, 1024, 'yes', 0, 'collect', 1, 1, 0),
        (0, 0, 1024, 'yes', 4096, 'collect', 1, 1, 0),
        (0, 0, 1024, 'yes', 4096, '-', 1, 1, 1),
        (0, 0, 1024, 'yes', 0, 'collect', 1, 1, 0),
        (0, 0, 1024, 'yes', 4096, 'collect', 1, 1, 0),
    ],
}


def child():
    """The scripted sequence (runs in the child process: python tests/test_gpu_frame_state.py)."""
    sys.path.insert(0, os.path.join(ROOT, "gaussian-ray-tracing_amd", "python"))
    import numpy as np
    import torch
    import grt

    def mark(step):  # (straight to the descriptor the library's fprintf(stderr) writes to: the two stay in order)
        os.write(2, f"## {step}\n".encode())

    def frames(n, fn):
        for _ in range(n):
            fn()
            torch.cuda.synchronize()

    steps = dict(SCRIPT)
    raw = grt.synth_scene(71, N)
    raw["scale"] = raw["scale"] + np.float32(0.5)
    acts = grt.activate(raw)
    center = grt.gaussian_center(acts["pos"])
    p = grt.default_params(W, H, center)
    q = grt.default_params(W, H, center, eye=(1.2, 0.5, 2.4))
    u8 = torch.zeros((H, W, 3), dtype=torch.uint8, device="cuda:0")
    tr = grt.Tracer(0)
    tr.upload(acts)
    mark("standing")
    frames(steps["standing"], lambda: tr.render(p, out_u8=u8))
    mark("move")
    frames(steps["move"], lambda: tr.render(q, out_u8=u8))
    mark("window")
    frames(steps["window"], lambda: tr.render(q, window=(0, 0, 128, 128), out_u8=u8))
    mark("tiles")
    t8 = torch.zeros((8, 64, 64, 3), dtype=torch.uint8, device="cuda:0")
    frames(steps["tiles"], lambda: tr.render_tiles(q, 64, 64, 1, 2, 8, out_u8=t8))
    mark("rays")
    rng = np.random.default_rng(5)
    eye = np.float32(list(p.eye))
    d = (np.float32(center) - eye)[None, :] + rng.normal(0.0, 0.4, (4096, 3)).astype(np.float32)
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    rays = torch.tensor(np.concatenate([np.broadcast_to(eye, d.shape), d], axis=1).astype(np.float32), device="cuda:0")
    frames(steps["rays"], lambda: tr.render_rays(p, rays))
    frames(4, lambda: tr.render(p, out_u8=u8))  # (unmarked lines are not compared: the standing view, settled again)
    mark("option")
    tr.set_option(grt.OPT_TILE_PARTS4_PCT, 50)
    frames(steps["option"], lambda: tr.render(p, out_u8=u8))
    mark("feedback0")
    tr.set_option(grt.OPT_FEEDBACK, 0)
    frames(steps["feedback0"] - 1, lambda: tr.render(p, out_u8=u8))
    tr.set_option(grt.OPT_FEEDBACK, 1)
    frames(1, lambda: tr.render(p, out_u8=u8))
    frames(4, lambda: tr.render(p, out_u8=u8))
    mark("upload")
    tr.upload(acts)
    frames(steps["upload"], lambda: tr.render(p, out_u8=u8))
    frames(4, lambda: tr.render(p, out_u8=u8))
    mark("view")
    v = tr.view()
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        frames(steps["view"] - 1, lambda: v.render(q, out_u8=u8))
    frames(1, lambda: tr.render(p, out_u8=u8))
    v.close()
    mark("aux_mesh")
    tr.set_meshes([grt.plane_mesh((float(center[0]), float(center[1]), float(center[2])))])
    frames(2, lambda: tr.render(p, out_u8=u8))
    frames(1, lambda: tr.render_aux(p, want_u8=False, want_f32=True))
    frames(steps["aux_mesh"] - 3, lambda: tr.render(p, out_u8=u8))
    tr.check()
    tr.close()


def parse(stderr):
    """{step: [fields of each `grt launch:` line]} of the child's stderr."""
    out, step, slots = {}, None, {}
    for line in stderr.splitlines():
        if line.startswith("## "):
            step = line[3:].strip()
            out[step] = []
        elif line.startswith("grt launch: ") and step is not None:
            w = line.split()
            f = dict(zip(w[2::2], w[3::2]))
            slot = slots.setdefault(f["ctx"], len(slots))
            out[step].append((slot, int(f["mode"]), int(f["units"]), f["order"], int(f["entries"]), f["cost"], int(f["parts_ok"]),
                              int(f["cost_valid"]), int(f["order_ready"])))
    return out


def run_child():
    env = dict(os.environ, GRT_DEBUG_LAUNCH="1")
    r = subprocess.run([sys.executable, os.path.abspath(__file__)], capture_output=True, text=True, timeout=300, env=env, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-4000:]
    return r.stderr


@pytest.mark.gpu
def test_frame_slot_state_frame_by_frame():
    got = parse(run_child())
    for step, n in SCRIPT:
        print(step, got.get(step))
    assert list(got) == [s for s, _ in SCRIPT]
    for step, n in SCRIPT:
        assert len(got[step]) >= n, step
        assert got[step][:n] == EXPECTED[step], step
    # the standing view: from the frame at which the costs stop being collected, every line is the same
    st = got["standing"]
    first_kept = next(i for i, f in enumerate(st) if f[5] == "-")
    assert first_kept >= 2 and all(f == st[first_kept] for f in st[first_kept:])
    assert all(f[3] == "yes" and f[5] == "collect" for f in st[:first_kept])


if __name__ == "__main__":
    child()
