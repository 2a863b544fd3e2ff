#!/usr/bin/env python3
"""`make detect`: a folder or a list of pictures through the pipeline - detections.json and annotated pictures, boxes and labels drawn
on the GPU (k210_yolo_framework_amd/detect.py).  keras_inference.py:137-174 for many pictures at once."""
from k210_yolo_framework_amd.detect import cli

if __name__ == '__main__':
    cli()
