#!/usr/bin/env python3
"""Launcher next to the reference's command scripts (`cd ../vision_benchmark; python commands/<command>.py --ds ... --model ...`):
`python commands/predict.py --ds resources/datasets/<d>.yaml --model resources/model/<m>.yaml --adapter <file>` scores a test
split with a saved adapter.  Not a reference command; the work is pevit_amd.commands.predict."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))

from pevit_amd.commands.predict import main  # noqa: E402

if __name__ == "__main__":
    main()
