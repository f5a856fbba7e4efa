"""python -m sibelia_amd: the reference program's command line over the library (see sibelia_amd/pipeline.py)."""
import sys

from .pipeline import main

if __name__ == "__main__":
    sys.exit(main())
