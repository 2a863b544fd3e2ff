#!/usr/bin/env python3
"""`make eval`: VOC mAP of a checkpoint, network and metric on the GPU (k210_yolo_framework_amd/evaluate.py).  The reference has no evaluator."""
from k210_yolo_framework_amd.evaluate import cli

if __name__ == '__main__':
    cli()
