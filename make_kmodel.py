from k210_yolo_framework_amd.make_kmodel import cli

if __name__ == '__main__':
    cli()
