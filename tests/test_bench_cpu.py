"""No GPU: the pieces of bench.py that decide what a record may contain (VERDICT r05 item 4b and the parity sub-record)."""
import importlib
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def test_bench_refuses_child_processes_under_a_profiler(monkeypatch):
    """Under rocprofv3 the profiler's preloaded library has initialised the GPU before bench.py starts: the cold jobs (child processes) must not run then."""
    bench = importlib.import_module("bench")
    for k in list(os.environ):
        if k.startswith(("ROCPROFILER_", "ROCP_", "ROCPROF_")):
            monkeypatch.delenv(k)
    monkeypatch.delenv("LD_PRELOAD", raising=False)
    assert not bench.profiler_attached()
    monkeypatch.setenv("ROCPROFILER_REGISTER_FORCE_LOAD", "1")
    assert bench.profiler_attached()
    monkeypatch.delenv("ROCPROFILER_REGISTER_FORCE_LOAD")
    monkeypatch.setenv("LD_PRELOAD", "/opt/rocm/lib/librocprofiler-sdk-tool.so")
    assert bench.profiler_attached()


def test_film_crc_is_a_function_of_the_crop_bits_only():
    bench = importlib.import_module("bench")
    rng = np.random.default_rng(1)
    film = rng.random((1084, 1924, 4), dtype=np.float32)
    a = bench.film_crc(film, 2)
    other = film.copy(); other[0, 0, 0] += 1.0                             # outside the crop: the same crc
    assert bench.film_crc(other, 2) == a and len(a) == 8
    other[508 + 2 + 10, 928 + 2 + 10, 1] = np.nextafter(other[508 + 2 + 10, 928 + 2 + 10, 1], np.float32(2.0))      # one bit inside the crop: another crc
    assert bench.film_crc(other, 2) != a
    assert bench.PARITY_CRC_N1 is not None and bench.PARITY_SPP_TABLE == bench.SPP


def test_profile_facts_are_stamped_with_the_live_sources():
    """profiles/pmc_latest.json describes ONE build: bench.py quotes its counter facts only when the kernel / ABI sources hash to the stamp (the last thing a round does
    to those sources is the profile run)."""
    import json
    import pytest
    bench = importlib.import_module("bench")
    facts = json.load(open(os.path.join(ROOT, "profiles", "pmc_latest.json")))
    if facts["source_sha16"] != bench.source_hash():                       # (not a failure of the product: bench.py then withholds the counter facts and says why)
        pytest.skip("kernel or ABI sources changed after the profile was taken: run scripts/profile_bench.sh + scripts/summarize_profile.py")
    assert os.path.isdir(os.path.join(ROOT, facts["profile"])) and "kz_wf_trace<0>" in facts["kernels"]


def test_dump_outputs_are_whole_or_a_fixed_sample_within_the_budget(tmp_path):
    """--dump-outputs: the C4 film + image are written whole; larger outputs (C5) as the same seeded sample of pixels in every run, the files within the budget."""
    bench = importlib.import_module("bench")
    rng = np.random.default_rng(2)
    film, rgb = rng.random((1084, 1924, 4), dtype=np.float32), rng.random((1080, 1920, 3), dtype=np.float32)
    assert bench.dump_outputs(str(tmp_path / "c4"), {"film": film, "rgb": rgb}) == {"film": [1084, 1924, 4], "rgb": [1080, 1920, 3]}
    for name, a in (("film", film), ("rgb", rgb)):
        b = np.load(tmp_path / "c4" / (name + ".npy"))
        assert b.dtype == np.float32 and np.array_equal(b, a), name
    film5, rgb5 = rng.random((2164, 3844, 4), dtype=np.float32), rng.random((2160, 3840, 3), dtype=np.float32)
    for run in ("a", "b"):
        shapes = bench.dump_outputs(str(tmp_path / run), {"film": film5, "rgb": rgb5})
        assert sum(os.path.getsize(tmp_path / run / f) for f in os.listdir(tmp_path / run)) <= bench.DUMP_BYTES
    for f in ("film.npy", "film_pixels.npy", "rgb.npy", "rgb_pixels.npy"):
        assert np.array_equal(np.load(tmp_path / "a" / f), np.load(tmp_path / "b" / f))
    idx = np.load(tmp_path / "a" / "rgb_pixels.npy").astype(np.int64)
    assert shapes["rgb"] == [len(idx), 3] and np.array_equal(np.load(tmp_path / "a" / "rgb.npy"), rgb5.reshape(-1, 3)[idx])


def test_only_a_full_run_starts_the_cold_jobs(monkeypatch):
    """A plain run goes straight to the headline figure: the cold jobs (child processes, before the GPU is touched) run with --full only. Without a GPU both runs
    then stop at the GPU check."""
    import pytest
    import torch
    bench = importlib.import_module("bench")
    started = []
    monkeypatch.setattr(bench, "run_cold_jobs", lambda tris: started.append(tris) or {})
    monkeypatch.setattr(bench, "profiler_attached", lambda: False)
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    saved = os.dup(1)                                                     # (main() points file descriptor 1 at stderr: the record goes to a copy of the original)
    try:
        for extra, cold in (([], []), (["--full"], [bench.NTRIS])):
            started.clear()
            monkeypatch.setattr(sys, "argv", ["bench.py", "--gpus", "1", "--steps", "1", "--warmup", "0"] + extra)
            with pytest.raises(SystemExit, match="needs a GPU"):
                bench.main()
            assert started == cold, extra
    finally:
        os.dup2(saved, 1)
        os.close(saved)
