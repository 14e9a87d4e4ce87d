"""The multi-clip command line's host logic (cli.py): grouping, batch sizes, clip order, output paths, refused modes."""
import os

import pytest

import fdcap_amd  # noqa: F401
from fdcap_amd import cli


def test_clips_are_grouped_by_scene_and_length_in_input_order():
    clips = [("a", 300), ("b", 300), ("a", 300), ("a", 200), ("a", 300), ("b", 300), ("a", 200)]
    assert cli.plan_batches(clips, clips_per_batch=2) == [("a", 300, [0, 2]), ("a", 300, [4]), ("b", 300, [1, 5]),
                                                          ("a", 200, [3, 6])]


def test_default_batch_size_is_the_largest_under_the_row_cap():
    assert cli.MULTICLIP_ROW_CAP == 1024
    assert cli.batch_size(300) == 3
    assert cli.batch_size(256) == 4
    assert cli.batch_size(1024) == 1 and cli.batch_size(5000) == 1
    assert cli.batch_size(300, clips_per_batch=8) == 8
    assert cli.batch_size(40, row_cap=200) == 5
    clips = [("s", 300)] * 7
    assert [b[2] for b in cli.plan_batches(clips)] == [[0, 1, 2], [3, 4, 5], [6]]
    assert all(len(b[2]) * b[1] <= cli.MULTICLIP_ROW_CAP for b in cli.plan_batches(clips))


def test_paths_follow_the_one_clip_form():
    bp = "/data/segmented/video7-3/"
    assert cli.sample_name_of(bp) == "video7-3"
    name, scene, cam = cli.clip_paths(bp, "/scenes")
    assert (name, scene, cam) == ("video7-3", os.path.join("/scenes", "video7-3", "meshed-poisson.ply"),
                                  os.path.join("/scenes", "video7-3", "camerapose.txt"))
    assert cli.clip_output_dir("/out", bp) == os.path.join("/out", "video7-3")


@pytest.mark.parametrize("mode", ["local", "dct"])
def test_modes_other_than_global_are_refused(mode, capsys):
    with pytest.raises(SystemExit) as e:
        cli.main(["--clips", "/x/a/", "/x/b/", "--fit-root", "/tmp/never", "--mode", mode])
    assert e.value.code != 0
    assert "global" in capsys.readouterr().err


def test_the_multi_clip_form_needs_a_fit_root(capsys):
    with pytest.raises(SystemExit):
        cli.main(["--clips", "/x/a/"])
    assert "--fit-root" in capsys.readouterr().err
