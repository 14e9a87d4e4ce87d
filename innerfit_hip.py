#!/usr/bin/env python3
"""`python3 innerfit_hip.py <keypoint_dir> <body_path>` -- the per-frame inner fit from OpenPose's JSON files to the
`<body_path>/results/*/*.pkl` that global_optimization_hip.py reads, on the MI355X path (fdcap_amd.cli_innerfit)."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import fdcap_amd  # noqa: E402,F401
from fdcap_amd.cli_innerfit import main  # noqa: E402

if __name__ == "__main__":
    sys.exit(main())
