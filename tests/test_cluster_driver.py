"""The offline driver's --clusters and --residue modes (erasor_offline_demo): bad arguments end with status 2 before anything is read or
launched, without a GPU.  (The modes' output on a GPU: tests/test_gpu_cluster.py.)"""
import subprocess

import pytest

from test_label_scans_driver import DEMO, ensure_demo


def run(*args):
    return subprocess.run([DEMO] + list(args), capture_output=True, timeout=60).returncode


@pytest.mark.parametrize("args", [
    ("--clusters",), ("--clusters", "cloud.pcd"), ("--clusters", "cloud.pcd", "0"), ("--clusters", "cloud.pcd", "-0.5"), ("--clusters", "cloud.pcd", "nan"),
    ("--clusters", "cloud.pcd", "inf"), ("--clusters", "cloud.pcd", "half"), ("--clusters", "cloud.pcd", "0.5x"), ("--clusters", "cloud.pcd", "0.5", "-1"),
    ("--clusters", "cloud.pcd", "0.5", "2.5"), ("--clusters", "cloud.pcd", "0.5", "2", "many"), ("--clusters", "cloud.pcd", "0.5", "2", "0", "kept.pcd", "more"),
])
def test_bad_clusters_arguments_exit_with_status_2(args):
    ensure_demo()
    assert run(*args) == 2


@pytest.mark.parametrize("args", [
    ("--residue",), ("--residue", "gt.pcd"), ("--residue", "gt.pcd", "est.pcd", "0"), ("--residue", "gt.pcd", "est.pcd", "tol"),
    ("--residue", "gt.pcd", "est.pcd", "0.5", "-0.2"), ("--residue", "gt.pcd", "est.pcd", "0.5", "0.2", "-1"),
    ("--residue", "gt.pcd", "est.pcd", "0.5", "0.2", "0", "more"),
])
def test_bad_residue_arguments_exit_with_status_2(args):
    ensure_demo()
    assert run(*args) == 2


def test_a_missing_cloud_is_not_a_usage_error():
    ensure_demo()
    assert run("--clusters", "/nonexistent/cloud.pcd", "0.5") == 3
