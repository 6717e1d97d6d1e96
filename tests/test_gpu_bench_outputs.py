"""bench.py --dump-outputs: a plain run writes what its last timed step computed as float32 / float64 .npy files, the
same arrays whatever the (timed, not counted) pre-roll ran before them, and prints the headline line only; nothing that
belongs behind --full runs.  Two small runs (64 streams) side by side, with different pre-rolls."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT

pytestmark = pytest.mark.gpu

BENCH = os.path.join(ROOT, "bench.py")
STREAMS, N, STEPS = 64, 16384, 4
NAMES = {"sample_streams", "spectra", "records", "pcm", "pulse_spectral", "pulse_audio"}


@pytest.fixture(scope="module")
def runs(tmp_path_factory):
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")}
    procs = []
    for prewarm in ("0", "40"):
        d = str(tmp_path_factory.mktemp("dump" + prewarm))
        cmd = [sys.executable, BENCH, "--gpus", "1", "--steps", str(STEPS), "--warmup", "2", "--streams", str(STREAMS),
               "--prewarm-ms", prewarm, "--dump-outputs", d]
        procs.append((d, subprocess.Popen(cmd, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, env=env)))
    out = []
    for d, p in procs:
        so, se = p.communicate(timeout=120)
        assert p.returncode == 0, se[-2000:]
        line = json.loads(so.strip().splitlines()[-1])
        out.append((line, {f[:-4]: np.load(os.path.join(d, f)) for f in os.listdir(d)}))
    return out


def test_plain_line_is_the_headline_only(runs):
    for line, _ in runs:
        assert line["steps"] == STEPS and line["unit"] == "IQ Msamples/s" and line["higher_is_better"] is True
        assert line["ms_per_step"] > 0
        # value and ms_per_step describe the same timed steps (the line rounds ms_per_step to 1e-4 ms, under 1 % of
        # a step of 64 frames, whose SSB chain alone takes 0.18 ms)
        assert line["value"] == pytest.approx(STREAMS * N / (line["ms_per_step"] * 1e-3) / 1e6, rel=2e-2)
        for key in ("cpu_baseline", "labelled", "roofline_isolated", "hbm_measured", "ssb_latency_floor"):
            assert key not in line, key


def test_dumped_outputs_are_the_last_steps_and_repeat(runs):
    (_, a), (_, b) = runs
    assert set(a) == set(b) == NAMES
    for name in NAMES:
        assert a[name].dtype in (np.float32, np.float64), name
        np.testing.assert_array_equal(a[name], b[name], err_msg=name)  # NaNs (none expected) compare equal here
    assert sum(v.nbytes for v in a.values()) <= 64 * 10**6
    rows = a["sample_streams"].astype(int)
    assert a["spectra"].shape == (len(rows), N) and len(set(rows)) == len(rows) and rows.max() < STREAMS
    assert a["records"].shape[0] == a["pcm"].shape[0] == a["pulse_audio"].shape[0] == STREAMS
    # computed, not left empty: power spectra with a tone far above the noise
    assert np.all(np.isfinite(a["spectra"])) and np.all(a["spectra"].max(axis=1) > 100 * np.median(a["spectra"], axis=1))
    import sdrg
    names = sdrg.RECORD_DTYPE.names
    # the statistics' peak is the spectrum's maximum inside the focus window
    lo, cnt = sdrg.focus_window(2_000_000, N, 5)
    peak = a["records"][rows, names.index("peak_bin")].astype(int)
    np.testing.assert_array_equal(peak, lo + np.argmax(a["spectra"][:, lo:lo + cnt], axis=1))
    assert np.any(a["pcm"] != 0) and np.all(a["pcm"] == np.round(a["pcm"])) and np.abs(a["pcm"]).max() <= 32768
