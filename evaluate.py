"""CLI shim: `python evaluate.py --hr_dir D [--model a.pt ...]` (see fast-srgan_amd/evaluate.py)."""
import importlib

if __name__ == "__main__":
    importlib.import_module("fast-srgan_amd.evaluate").main()
