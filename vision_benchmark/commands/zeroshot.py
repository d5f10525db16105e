#!/usr/bin/env python3
"""Launcher at the path the reference's scripts use:
`cd ../vision_benchmark; python commands/zeroshot.py --ds resources/datasets/<d>.yaml --model resources/model/<m>.yaml ...`
(reference: vision_benchmark/commands/zeroshot.py).  Same flags and outputs; the work is pevit_amd.commands.zeroshot."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))

from pevit_amd.commands.zeroshot import main  # noqa: E402

if __name__ == "__main__":
    main()
