"""CLI shim: `python video.py --input IN --output OUT` (Y4M I420 streams; see fast-srgan_amd/video.py)."""
import importlib

if __name__ == "__main__":
    importlib.import_module("fast-srgan_amd.video").main()
