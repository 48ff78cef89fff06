# builds the C++ mirror of the dense step (tests/test_dense_gpu.py, tests/test_dense_cpu.py) against the in-tree libsfmhip.so
dense_test: dense_test.cpp ../../sfm_opencv_amd/host/sfm_ops.hpp ../../include/sfmhip.h
	g++ -O2 -std=c++17 -Wall -o $@ dense_test.cpp -L../../sfm_opencv_amd -lsfmhip -Wl,-rpath,'$$ORIGIN/../../sfm_opencv_amd' -Wl,-rpath,/opt/rocm/lib
