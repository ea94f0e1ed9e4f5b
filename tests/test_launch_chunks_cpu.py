"""launch_chunks (csrc/srg_internal.h) walks every kernel family's grid in launch-sized chunks.  The walk itself
is checked on the host: tests/launch_chunks_main.cpp drives it with a recording callable (no GPU call) and
asserts that the chunks tile [0, blocks) in ascending order, that none is empty or larger than a launch,
and that a non-zero status at the second chunk stops the walk there and is returned.

The caps of most families correspond to tens of millions of rows; the GPU tests reach a second chunk through
the test hook srg_debug_launch_cap, which bounds the blocks of one launch (tests/test_launch_chunks_gpu.py
runs every chunked entry across chunk boundaries against its CPU reference).  The same host program checks
the hook's side of the walk, launch_chunks_capped: under an override of 3 a walk over 8 blocks makes the
chunks 3, 3, 2 and the launch counter rises by 3; an override above the site's default does not raise it;
removing the override restores the default; a failing chunk still stops the walk."""
import os
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")


def test_launch_chunks_tiles_the_grid_and_stops_at_the_first_failure(tmp_path):
    exe = str(tmp_path / "launch_chunks_main")
    # (a named target: hipcc otherwise spends seconds looking for a GPU to compile for)
    build = subprocess.run([HIPCC, "-O2", "-std=c++17", "--offload-arch=gfx950", "-I", os.path.join(REPO, "include"),
                            "-I", os.path.join(REPO, "scalable-roubust-gnn_amd", "csrc"), "-o", exe,
                            os.path.join(HERE, "launch_chunks_main.cpp")], capture_output=True, text=True, timeout=300)
    assert build.returncode == 0, build.stdout + build.stderr
    run = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert run.returncode == 0, run.stdout + run.stderr
    lines = [ln for ln in run.stdout.splitlines() if ln.startswith("blocks=")]
    capped = [ln for ln in run.stdout.splitlines() if ln.startswith("capped ")]
    assert len(lines) + len(capped) == len(run.stdout.splitlines()), run.stdout
    assert capped == [f"capped {k}=ok" for k in ("default", "override3", "stops", "no_raise", "restored")], run.stdout
    assert [ln.split()[0] for ln in lines] == [f"blocks={b}" for b in (0, 1, 3, 4, 5, 8, 9)], run.stdout
    assert all(ln.endswith("tiles=ok stops=ok") for ln in lines), run.stdout
