#!/usr/bin/env python3
"""Launcher at the path the reference's scripts use: scripts/run.sh (mode linear_probe) does
`cd ../vision_benchmark; python commands/linear_probe.py --ds resources/datasets/<d>.yaml --model resources/model/<m>.yaml ...`
(reference: vision_benchmark/commands/linear_probe.py).  Same flags and outputs; the work is pevit_amd.commands.linear_probe."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))

from pevit_amd.commands.linear_probe import main  # noqa: E402

if __name__ == "__main__":
    main()
