# builds the C++ mirror of the mesh clean-up (tests/test_mesh_gpu.py) against the in-tree libsfmhip.so
mesh_test: mesh_test.cpp ../../sfm_opencv_amd/host/sfm_ops.hpp ../../include/sfmhip.h
	g++ -O2 -std=c++17 -Wall -o $@ mesh_test.cpp -L../../sfm_opencv_amd -lsfmhip -Wl,-rpath,'$$ORIGIN/../../sfm_opencv_amd' -Wl,-rpath,/opt/rocm/lib
